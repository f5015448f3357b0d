"""``python -m nuts333_amd.devpath --input K[,K...]``: input_many over raw reads timed beside speak_many of the same
events parsed beforehand, and beside the CPU parsing them.

Host tier: the option rejects what ``--per-call`` rejects; with no GPU visible the command still exits 2 and measures
nothing; the reads it times parse into the events ``--speak`` times.  GPU tier: the command, at a small repetition
count, in one short-lived child under ``timeout``, prints one line whose ``input`` section has a case per colour and K
with both sides' times and a download that grows with K alone.  No time is a pass condition.
"""
from __future__ import annotations

import json

import pytest

import child_run
from device_input_child import SPEECH, answer_of
from nuts333_amd import device, devpath


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "10,-3", "x", "1,x", "", "1,,2", "2.5"])
def test_input_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--input", value])
    assert e.value.code == 2
    assert "argument --input:" in capsys.readouterr().err


def test_input_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "input_cases", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--input", "1,10"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_input_cases_have_no_cpu_fall_back(monkeypatch):
    def refuse():
        raise RuntimeError("no GPU")
    monkeypatch.setattr(device, "_load", refuse)
    with pytest.raises(RuntimeError, match="no GPU"):
        devpath.input_cases([1], 1, 0, {"format_line_once_ns": 1.0})


def test_the_timed_reads_parse_into_the_events_speak_times():
    speaker = {"slot": 0, "room": 0, "name": b"Uaaa", "vis": 1, "muzzled": 0, "command_mode": 0, "level": 1}
    reads, events = devpath.input_reads(12), devpath.speak_events(12)
    for (slot, data), (eslot, com, inpstr, wc) in zip(reads, events):
        d, m = answer_of(speaker, data, True)
        assert slot == eslot == 0 and d["kind"] == SPEECH and not d["forced"]
        assert (d["com"], data[d["start"]:d["start"] + d["size"]], d["word_count"]) == (com, inpstr, wc)
    assert [answer_of(speaker, data, True)[1]["line"] for _, data in reads] == devpath.line_texts("say", 12)
    for exec_com in (False, True):
        cpu = devpath.input_cpu_us(reads, 3, 1, exec_com)
        assert 0 < cpu["p10"] <= cpu["median"] <= cpu["p90"]
    assert [data for _, data in reads] == [data for _, data in devpath.input_reads(12)]      # the timing cut no read


@pytest.mark.gpu
def test_devpath_input_prints_one_line_with_both_sides(built):
    j = child_run.run_devpath("devpath --input", 600, "--input", "1,8,64",
                              "--reps", "10", "--warmup", "2", "--pathbench-iterations", "200000")
    assert len(j["cases"]) == 18 and not {"plan", "roster", "per_call", "review", "speak"} & set(j)
    assert j["input_kernels"] == ["nuts_roster_parse", "nuts_roster_speak", "nuts_roster_speak_plan"]
    assert set(j["input_kernels"]) <= set(device.KERNELS) and j["input_end_to_end_covers"] and j["input_cpu_us_covers"]
    ip = j["input"]
    assert [(c["colour"], c["k"]) for c in ip] == [(colour, k) for colour in devpath.COLOURS for k in (1, 8, 64)]
    for c in ip:
        assert c["n"] == 1000 and c["recipients"] == c["k"] * 999
        for side in (c, c["speak_many_of_the_parsed_events"]):
            assert 0 < side["kernels_us"]["median"] <= side["end_to_end_us"]["median"] <= side["python_us"]["median"]
            assert side["h2d_bytes"] > 0 and side["d2h_bytes"] > 0
        assert c["d2h_bytes"] > c["speak_many_of_the_parsed_events"]["d2h_bytes"]             # what the parse found, too
        assert set(c["parsing_adds_us"]) == {"kernels_us", "end_to_end_us", "python_us"}
        assert c["cpu_us"]["median"] > 0 and c["cpu_exec_com_us"]["median"] > 0
    by_k = {k: {c["d2h_bytes"] for c in ip if c["k"] == k} for k in (1, 8, 64)}
    assert all(len(v) == 1 for v in by_k.values())                                          # with K alone
    assert min(by_k[1]) < min(by_k[8]) < min(by_k[64])
    print("\n[devpath --input]", json.dumps(ip)[:3000])
