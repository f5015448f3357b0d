"""``python -m nuts333_amd.devpath --plan K[,K...]``: delivery plans for a resident roster, timed beside ``--roster``.

Host tier: the option rejects what ``--per-call`` rejects, and with no GPU visible the command still exits 2 and
measures nothing.  GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``,
prints one line; a plan uploads the same bytes per call whatever the roster's size, costs less end to end and less
Python than the ``roster`` case of the same command at N = 1000, K = 100, and amortises its per-call cost.
"""
from __future__ import annotations

import json

import pytest

import child_run
from nuts333_amd import devpath


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "10,-3", "x", "1,x", "", "1,,2", "2.5"])
def test_plan_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--plan", value])
    assert e.value.code == 2
    assert "argument --plan:" in capsys.readouterr().err       # the option's own check, not an unknown option


def test_plan_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "roster_case", lambda *a, **k: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "plan_case", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--plan", "1,10"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


@pytest.mark.gpu
def test_devpath_plan_prints_one_line_and_beats_the_roster(built):
    line = child_run.run_devpath_line("devpath --plan", 600, "--roster", "100",
                                       "--plan", "1,100", "--reps", "10", "--warmup", "2", "--pathbench-iterations", "200000")
    j = json.loads(line)
    assert "nuts_roster_plan" in j["plan_kernels"] and j["plan_end_to_end_covers"]
    pl = j["plan"]
    assert len(pl) == 36 and {(c["n"], c["text"], c["colour"], c["k"]) for c in pl} == {
        (n, t, c, k) for n in (10, 100, 1000) for t in ("say", "shout") for c in ("off", "on", "half") for k in (1, 100)}
    for c in pl:
        assert c["recipients"] == c["k"] * (c["n"] - 1) and c["bytes_out"] > 0 and c["writes"] >= c["recipients"]
        assert c["cpu_derived_us"] > 0 and c["d2h_bytes"] > 0
        assert 0 < c["kernels_us"]["median"] <= c["end_to_end_us"]["median"] <= c["python_us"]["median"]
        assert c["h2d_bytes_first_call"] > c["h2d_bytes"] > 0
    h2d = {(c["text"], c["colour"], c["k"], c["n"]): c["h2d_bytes"] for c in pl}
    for (text, colour, k, n), b in h2d.items():
        if n == 1000:
            assert b == h2d[text, colour, k, 10], (text, colour, k)     # no table in a no-change call
    # the same cases through the arena path, measured in the same command: the plan does a subset of its work
    ro = {(c["text"], c["colour"]): c for c in j["roster"] if c["n"] == 1000 and c["k"] == 100}
    e2e = {(c["text"], c["colour"], c["k"]): c["end_to_end_us_per_broadcast"]["median"] for c in pl if c["n"] == 1000}
    assert len(ro) == 6
    for c in pl:
        if c["n"] == 1000 and c["k"] == 100:
            r = ro[c["text"], c["colour"]]
            print(f"\n[plan vs roster] {c['text']}/{c['colour']}: end to end per broadcast "
                  f"{c['end_to_end_us_per_broadcast']['median']} vs {r['end_to_end_us_per_broadcast']['median']} us, "
                  f"python {c['python_us_per_broadcast']['median']} vs {r['python_us_per_broadcast']['median']} us, "
                  f"d2h {c['d2h_bytes']} vs {r['d2h_bytes']} bytes")
            assert c["bytes_out"] == r["bytes_out"] and c["writes"] == r["writes"]
            assert c["end_to_end_us_per_broadcast"]["median"] < r["end_to_end_us_per_broadcast"]["median"], c
            assert c["python_us_per_broadcast"]["median"] < r["python_us_per_broadcast"]["median"], c
            assert e2e[c["text"], c["colour"], 100] < 0.5 * e2e[c["text"], c["colour"], 1], (c["text"], e2e)
    print("\n[devpath --plan]", line[:800])
