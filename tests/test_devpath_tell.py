"""``python -m nuts333_amd.devpath --tell K[,K...]``: tell_many timed beside speak_many of says of the same bodies.

Host tier: the option rejects what ``--per-call`` rejects; with no GPU visible the command still exits 2 and measures
nothing; the events it times are tells the model answers TOLD, to the one target, over the bodies the ``speak`` section
says.  GPU tier: the command, at a small repetition count, in one short-lived child under ``timeout``, prints one line
whose ``tell`` section has a case per colour and K with both sides' times and a download that grows with K alone.  No
time is a pass condition.
"""
from __future__ import annotations

import json

import pytest

import child_run
from device_tell_child import TOLD, new_user, private
from nuts333_amd import device, devpath


@pytest.mark.parametrize("value", ["0", "-1", "1,0", "10,-3", "x", "1,x", "", "1,,2", "2.5"])
def test_tell_rejects_what_per_call_rejects(value, capsys):
    with pytest.raises(SystemExit) as e:
        devpath.main(["--tell", value])
    assert e.value.code == 2
    assert "argument --tell:" in capsys.readouterr().err


def test_tell_without_a_gpu_exits_2_and_measures_nothing(monkeypatch, capsys):
    monkeypatch.setattr(devpath.device, "device_count", lambda: 0)
    monkeypatch.setattr(devpath, "pathbench", lambda n: pytest.fail("measured without a GPU"))
    monkeypatch.setattr(devpath, "tell_cases", lambda *a, **k: pytest.fail("measured without a GPU"))
    assert devpath.main(["--reps", "1", "--tell", "1,10"]) == 2
    assert "no GPU visible" in capsys.readouterr().err


def test_tell_cases_have_no_cpu_fall_back(monkeypatch):
    def refuse():
        raise RuntimeError("no GPU")
    monkeypatch.setattr(device, "_load", refuse)
    with pytest.raises(RuntimeError, match="no GPU"):
        devpath.tell_cases([1], 1, 0, {"format_line_once_ns": 1.0})


def test_the_timed_events_are_tells_of_the_say_bodies_to_one_target():
    slot, name = devpath.TELL_TARGET
    users = {j: new_user(j, name=b"User%d" % j) for j in range(1000)}
    users[0]["name"], users[slot]["name"] = b"Uaaa", name
    tells, says = devpath.tell_events(12), devpath.speak_events(12)
    for (who, com, inpstr, wc), (_, _, body, _) in zip(tells, says):
        m = private(users, who, com, inpstr, wc)
        assert (who, com, m["outcome"], m["target"]) == (0, device.COM_TELL, TOLD, slot)
        assert m["line"] == b"~OLUaaa tells you:~RS " + body + b"\n" and m["reply"] == b"~OLYou tell Zebedee:~RS " + body + b"\n"


@pytest.mark.gpu
def test_devpath_tell_prints_one_line_with_both_sides(built):
    j = child_run.run_devpath("devpath --tell", 600, "--tell", "1,8,64",
                              "--reps", "10", "--warmup", "2", "--pathbench-iterations", "200000")
    assert len(j["cases"]) == 18 and not {"plan", "roster", "per_call", "review", "speak", "input"} & set(j)
    assert j["tell_kernels"] == ["nuts_roster_tell", "nuts_roster_speak_plan"] and j["tell_end_to_end_covers"]
    assert set(j["tell_kernels"]) <= set(device.KERNELS) and "estimate" in j["tell_cpu_derived_estimate_us_covers"]
    tl = j["tell"]
    assert [(c["colour"], c["k"]) for c in tl] == [(colour, k) for colour in devpath.COLOURS for k in (1, 8, 64)]
    for c in tl:
        assert c["n"] == 1000 and c["recipients"] == c["k"] and c["target"] == devpath.TELL_TARGET[0]
        for side in (c, c["speak_many_of_the_same_bodies"]):
            assert 0 < side["kernels_us"]["median"] <= side["end_to_end_us"]["median"] <= side["python_us"]["median"]
            assert side["h2d_bytes"] > 0 and side["d2h_bytes"] > 0
        assert set(c["tell_over_speak"]) == {"kernels_us", "end_to_end_us", "python_us"}
        assert c["cpu_derived_estimate_us"] > 0 and "cpu_us" not in c and "python_model_us" not in c
    by_k = {k: {c["d2h_bytes"] for c in tl if c["k"] == k} for k in (1, 8, 64)}
    assert all(len(v) == 1 for v in by_k.values())                                          # with K alone
    assert min(by_k[1]) < min(by_k[8]) < min(by_k[64])
    print("\n[devpath --tell]", json.dumps(tl)[:3000])
