"""``python -m nuts333_amd.devpath --per-call K[,K...]``: many broadcasts per device call.

Host tier: the option's parser rejects what is not a positive count, and with no GPU visible the command still exits 2
and measures nothing.  GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``,
prints one line with the 18 single-broadcast cases and the per-call cases, and batching amortises the per-call cost.
"""
from __future__ import annotations

import json

import pytest

import child_run
from nuts333_amd import devpath


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "10,-3", "x", "1,x", "", "1,,2", "2.5"])
def test_per_call_rejects_what_is_not_a_positive_count(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--per-call", value])
    assert e.value.code == 2
    assert "--per-call" in capsys.readouterr().err


def test_per_call_counts_parse():
    assert devpath.per_call_counts("1,10,100") == [1, 10, 100] and devpath.per_call_counts("7") == [7]


def test_per_call_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath.device, "broadcast_many", lambda calls: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--per-call", "1,10"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_line_texts_differ_only_in_their_line_number():
    texts = devpath.line_texts("shout", 100)
    assert len(set(texts)) == 100 and len({len(t) for t in texts}) == 1
    assert texts[0] == devpath.TEXTS["shout"].replace(b"000123", b"000000")
    assert texts[99] == devpath.TEXTS["shout"].replace(b"000123", b"000099")


@pytest.mark.gpu
def test_devpath_per_call_prints_one_line_and_amortises(built):
    line = child_run.run_devpath_line("devpath --per-call", 600, "--per-call", "1,100",
                                       "--reps", "10", "--warmup", "2", "--pathbench-iterations", "200000")
    j = json.loads(line)
    assert len(j["cases"]) == 3 * 2 * 3
    assert "nuts_fanout_measure_many" in j["per_call_kernels"] and "nuts_fanout_emit_many" in j["per_call_kernels"]
    pc = j["per_call"]
    assert len(pc) == 3 * 2 * 3 * 2
    assert {(c["n"], c["text"], c["colour"], c["k"]) for c in pc} == {
        (n, t, c, k) for n in (10, 100, 1000) for t in ("say", "shout") for c in ("off", "on", "half") for k in (1, 100)}
    for c in pc:
        assert c["recipients"] == c["k"] * (c["n"] - 1) and c["bytes_out"] > 0 and c["cpu_derived_us"] > 0
        assert 0 < c["kernels_us"]["median"] <= c["end_to_end_us"]["median"] <= c["python_us"]["median"]
        assert c["end_to_end_us_per_broadcast"]["median"] == pytest.approx(c["end_to_end_us"]["median"] / c["k"],
                                                                           abs=0.01)
    e2e = {(c["text"], c["colour"], c["k"]): c["end_to_end_us_per_broadcast"]["median"] for c in pc if c["n"] == 1000}
    for text in ("say", "shout"):
        for colour in ("off", "on", "half"):
            assert e2e[text, colour, 100] < 0.5 * e2e[text, colour, 1], (text, colour, e2e)
    print("\n[devpath --per-call]", line[:800])
