"""``python -m nuts333_amd.devpath --roster K[,K...]``: broadcasts to a resident roster, timed beside ``--per-call``.

Host tier: the option rejects what ``--per-call`` rejects, and with no GPU visible the command still exits 2 and
measures nothing.  GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``,
prints one line; the roster uploads the same bytes per call whatever its size, costs less Python than ``per_call`` and
amortises its per-call cost.
"""
from __future__ import annotations

import json

import pytest

import child_run
from nuts333_amd import devpath


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "10,-3", "x", "1,x", "", "1,,2", "2.5"])
def test_roster_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--roster", value])
    assert e.value.code == 2
    assert "argument --roster:" in capsys.readouterr().err     # the option's own check, not an unknown option


def test_roster_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "roster_case", lambda *a: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--roster", "1,10"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


@pytest.mark.gpu
def test_devpath_roster_prints_one_line_and_beats_per_call(built):
    line = child_run.run_devpath_line("devpath --roster", 600, "--per-call", "100",
                                       "--roster", "1,100", "--reps", "10", "--warmup", "2", "--pathbench-iterations", "200000")
    j = json.loads(line)
    assert "nuts_roster_measure" in j["roster_kernels"] and "nuts_roster_emit" in j["roster_kernels"]
    ro = j["roster"]
    assert {(c["n"], c["text"], c["colour"], c["k"]) for c in ro} == {
        (n, t, c, k) for n in (10, 100, 1000) for t in ("say", "shout") for c in ("off", "on", "half") for k in (1, 100)}
    for c in ro:
        assert c["recipients"] == c["k"] * (c["n"] - 1) and c["bytes_out"] > 0 and c["cpu_derived_us"] > 0
        assert 0 < c["kernels_us"]["median"] <= c["end_to_end_us"]["median"] <= c["python_us"]["median"]
        assert c["h2d_bytes_first_call"] > c["h2d_bytes"] > 0
    h2d = {(c["text"], c["colour"], c["k"], c["n"]): c["h2d_bytes"] for c in ro}
    for (text, colour, k, n), b in h2d.items():
        if n == 1000:
            assert b == h2d[text, colour, k, 10], (text, colour, k)     # no table in a no-change call
    py = {(c["text"], c["colour"]): c["python_us_per_broadcast"]["median"]
          for c in j["per_call"] if c["n"] == 1000 and c["k"] == 100}
    e2e = {(c["text"], c["colour"], c["k"]): c["end_to_end_us_per_broadcast"]["median"] for c in ro if c["n"] == 1000}
    for c in ro:
        if c["n"] == 1000 and c["k"] == 100:
            assert c["python_us_per_broadcast"]["median"] < py[c["text"], c["colour"]], c
            assert e2e[c["text"], c["colour"], 100] < 0.5 * e2e[c["text"], c["colour"], 1], (c["text"], e2e)
    print("\n[devpath --roster]", line[:800])
