"""``python -m nuts333_amd.devpath``: the device-path measurement command.

GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``,
returns one well-formed JSON line covering every case.  Host tier: with no GPU visible it exits non-zero with a
message and measures nothing -- there is no CPU fall-back.
"""
from __future__ import annotations

import json

import pytest

import child_run
from nuts333_amd import devpath


def test_devpath_without_a_gpu_exits_nonzero_and_says_why(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_cpu_derived_broadcast_cost_is_n_recipients_plus_one_format():
    pb = {"transduce_say_colour_off_ns": 50.0, "transduce_say_colour_on_ns": 60.0, "fanout_predicate_ns": 1.0,
          "format_line_once_ns": 40.0}
    assert devpath.cpu_derived_us(pb, "say", "off", 1000) == pytest.approx((999 * 50 + 1000 + 40) / 1e3)
    assert devpath.cpu_derived_us(pb, "say", "half", 10) == pytest.approx((9 * 55 + 10 + 40) / 1e3)


def test_listener_tables_have_one_sender_and_the_asked_colours():
    t = devpath.listeners(10, "half")
    f = devpath.device.LISTENER_FIELDS
    assert t.shape == (10, 7) and t[:, f.index("is_sender")].tolist() == [1] + [0] * 9
    assert t[:, f.index("colour")].tolist() == [0, 1] * 5
    assert devpath.listeners(3, "on")[:, f.index("colour")].tolist() == [1, 1, 1]


@pytest.mark.gpu
def test_devpath_command_prints_one_well_formed_json_line(built):
    line = child_run.run_devpath_line("devpath", 600, "--reps", "20", "--warmup", "5", "--pathbench-iterations", "200000")
    j = json.loads(line)
    assert j["reps"] == 20 and "nuts_fanout_measure_broadcast" in j["kernels"]
    assert len(j["cases"]) == 3 * 2 * 3
    assert {(c["n"], c["text"], c["colour"]) for c in j["cases"]} == {
        (n, t, c) for n in (10, 100, 1000) for t in ("say", "shout") for c in ("off", "on", "half")}
    for c in j["cases"]:
        assert c["recipients"] == c["n"] - 1 and c["bytes_out"] > 0 and c["cpu_derived_us"] > 0
        assert 0 < c["kernels_us"]["median"] <= c["end_to_end_us"]["median"]
        assert c["kernels_us"]["p10"] <= c["kernels_us"]["median"] <= c["kernels_us"]["p90"]
    print("\n[devpath]", line[:800])
