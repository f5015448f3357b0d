"""``python -m nuts333_amd.devpath --relay K[,K...]``: relay_many timed beside plan_many and the CPU doing clone_relay's work.

Host tier: the option rejects what ``--per-call`` rejects; with no GPU visible the command still exits 2 and measures
nothing; the broadcasts it times are says to room 0 whose relay texts fit the reference's buffer.
GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``, prints one line whose
``relay`` section has a case per colour, number of relaying clones and K with the device's times for both calls, the CPU's,
and what each figure covers.  No time is a pass condition.
"""
from __future__ import annotations

import json

import pytest

import child_run
from device_relay_child import longest_text, relay_text
from nuts333_amd import device, devpath


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "10,-3", "x", "1,x", "", "1,,2", "2.5"])
def test_relay_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--relay", value])
    assert e.value.code == 2
    assert "argument --relay:" in capsys.readouterr().err


def test_relay_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "relay_cases", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--relay", "1,8"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_relay_cases_have_no_cpu_fall_back(monkeypatch):
    def refuse():
        raise RuntimeError("no GPU")
    monkeypatch.setattr(device, "_load", refuse)
    with pytest.raises(RuntimeError, match="no GPU"):
        devpath.relay_cases([1], 1, 0, {})


def test_the_broadcasts_are_says_to_room_0_that_a_clone_can_relay():
    bs = devpath.relay_broadcasts(64)
    assert len(bs) == 64 and len({b[0] for b in bs}) == 64
    for text, rm, sender, force_listen, com in bs:
        assert (rm, sender, force_listen, com) == (0, 5, 0, device.COM_SAY) and sender % len(devpath.LOOK_ROOMS) == rm
        assert text.startswith(b"User5 says: ") and text.endswith(b"\n") and len(text) <= longest_text(devpath.LOOK_ROOMS[0])
        assert relay_text(devpath.LOOK_ROOMS[0], text).startswith(b"~FT[ drive ]:~RS User5 says: ")
    assert devpath.RELAY_CLONES == 64


@pytest.mark.gpu
def test_devpath_relay_prints_one_line_with_both_sides(built):
    j = child_run.run_devpath("devpath --relay", 600, "--relay", "1,8,64",
                              "--reps", "5", "--warmup", "1", "--pathbench-iterations", "200000")
    assert len(j["cases"]) == 18 and not {"plan", "roster", "per_call", "review", "speak", "input", "tell", "look"} & set(j)
    assert j["relay_kernels"] == ["nuts_roster_relay"] and set(j["relay_kernels"]) <= set(device.RELAY_KERNELS)
    assert "nuts_roster_plan" in j["relay_end_to_end_covers"] and "nuts_roster_speak_plan" in j["relay_end_to_end_covers"]
    assert "plan_many of the same K broadcasts" in j["relay_end_to_end_covers"]
    assert "np_contains_swearing" in j["relay_cpu_us_covers"] and "leaves the sprintf" in j["relay_cpu_us_covers"]
    rl = j["relay"]
    assert [(c["colour"], c["relaying_clones"], c["k"]) for c in rl] == [(colour, clones, k) for colour in devpath.COLOURS
                                                                         for clones in (0, 1, 64) for k in (1, 8, 64)]
    keys = {"n", "k", "colour", "relaying_clones", "relays", "relay_bytes_out", "kernels_us", "end_to_end_us", "python_us",
            "plan_kernels_us", "plan_end_to_end_us", "plan_python_us", "cpu_us", "h2d_bytes", "d2h_bytes", "plan_h2d_bytes",
            "plan_d2h_bytes", "end_to_end_over_plan", "end_to_end_over_cpu"}
    for c in rl:
        assert set(c) == keys and c["n"] == 1000 and c["relays"] == c["k"] * c["relaying_clones"]
        assert (c["relay_bytes_out"] > 0) == (c["relaying_clones"] > 0)
        assert (c["end_to_end_over_cpu"] is None) == (c["relaying_clones"] == 0)
        assert c["h2d_bytes"] > c["plan_h2d_bytes"] > 0 and c["d2h_bytes"] > c["plan_d2h_bytes"] > 0
        for f in ("kernels_us", "end_to_end_us", "python_us", "plan_kernels_us", "plan_end_to_end_us", "plan_python_us", "cpu_us"):
            assert set(c[f]) == {"median", "p10", "p90"}
    by_k = {k: {(c["h2d_bytes"], c["d2h_bytes"]) for c in rl if c["k"] == k} for k in (1, 8, 64)}
    assert all(len(v) == 1 for v in by_k.values())                      # the copies depend on the K texts alone
    print("\n[devpath --relay]", json.dumps(rl)[:3000])
