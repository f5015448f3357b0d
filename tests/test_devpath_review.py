"""``python -m nuts333_amd.devpath --review Q[,Q...]``: review_many timed beside the CPU doing the same lines, and what
``record`` adds to ``plan_many``.

Host tier: the option rejects what ``--per-call`` rejects and more rooms than a roster has rings; with no GPU visible
the command still exits 2 and measures nothing; without the option the command's output has no ``review`` section.
GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``, prints one line whose
``review`` section has a case per Q with both sides' times and a copy volume that grows with Q alone.  No time is a
pass condition.
"""
from __future__ import annotations

import json

import pytest

import child_run
from nuts333_amd import device, devpath


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "10,-3", "x", "1,x", "", "1,,2", "2.5",
                                   str(device.MAX_REVIEW_ROOMS + 1)])
def test_review_rejects_what_per_call_rejects_and_too_many_rooms(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--review", value])
    assert e.value.code == 2
    assert "argument --review:" in capsys.readouterr().err


def test_review_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "review_cases", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--review", "1,10"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_review_cases_have_no_cpu_fall_back(monkeypatch):
    def refuse():
        raise RuntimeError("no GPU")
    monkeypatch.setattr(device, "_load", refuse)
    with pytest.raises(RuntimeError, match="no GPU"):
        devpath.review_cases([1], 1, 0, {"transduce_say_colour_off_ns": 1.0, "transduce_say_colour_on_ns": 1.0})


@pytest.mark.gpu
def test_devpath_review_prints_one_line_with_both_sides(built):
    j = child_run.run_devpath("devpath --review", 600, "--review", "1,8,64",
                              "--reps", "10", "--warmup", "2", "--pathbench-iterations", "200000")
    assert len(j["cases"]) == 18 and "plan" not in j and "roster" not in j          # the other sections as they were
    assert j["review_kernels"] == ["nuts_roster_review"] and j["review_rings"] == 64
    assert "nuts_roster_record" in j["record_kernels"] and j["review_end_to_end_covers"]
    rv = j["review"]
    assert [c["q"] for c in rv] == [1, 8, 64]
    say = len(devpath.TEXTS["say"])
    for c in rv:
        assert c["lines"] == 15 * c["q"] and c["sequential"] == 0
        assert c["bytes_out"] == c["lines"] * ((say + 1) + (say + 1 + 4 + 4))      # "\n" -> "\n\r"; colour: two resets
        assert c["writes"] == c["lines"] * 3                                       # 1 with colour off, 2 with it on
        assert 0 < c["kernels_us"]["median"] <= c["end_to_end_us"]["median"] <= c["python_us"]["median"]
        assert c["cpu_us"]["median"] > 0 and c["cpu_derived_us"] > 0 and c["end_to_end_over_cpu"] > 0
        assert c["h2d_bytes"] > 0 and c["d2h_bytes"] >= c["q"] * 2 * device.MAX_REVIEW_BYTES
    assert rv[0]["d2h_bytes"] < rv[1]["d2h_bytes"] < rv[2]["d2h_bytes"]
    rec = j["record"]
    assert rec["k"] == 100 and rec["n"] == 1000
    for side in ("with_record", "without_record"):
        assert 0 < rec[side]["kernels_us"]["median"] <= rec[side]["end_to_end_us"]["median"]
    assert set(rec["record_adds_us"]) == {"kernels_us", "end_to_end_us", "python_us"}
    print("\n[devpath --review]", json.dumps({"review": rv, "record": rec})[:3000])
