"""``nuts333_amd.devpath._timed``: the one timed loop behind every section of the command.

Host tier only: the steps are plain callables whose results carry a hand-made ``timing``, so no GPU and no device library
is needed.  Each test fails if the loop is wrong in the way its name says: the order of the calls and which rounds are
kept, where the host clock is read, the copy-volume check in the kept rounds and in the warm-up, results without a copy
volume or without a timing, and the smallest run the sections' own tests ask for.
"""
from __future__ import annotations

from types import SimpleNamespace

import pytest

from nuts333_amd import devpath


def result(kernels_us=1.0, end_to_end_us=2.0, **copy):
    return SimpleNamespace(timing={"kernels_us": kernels_us, "end_to_end_us": end_to_end_us, **copy})


def test_rounds_run_every_step_in_order_and_only_the_last_reps_are_kept():
    log = []

    def step(name):
        def call():
            log.append(name)
            return result(kernels_us=float(len(log) - 1), end_to_end_us=100.0 + len(log) - 1)
        return call
    got = devpath._timed("order", {"A": step("A"), "B": step("B")}, reps=3, warmup=2)
    assert log == ["A", "B"] * 5
    assert list(got) == ["A", "B"]
    # call i of the log has kernels_us i: A's kept calls are 4, 6, 8 and B's 5, 7, 9 -- not 0 .. 8 or 1 .. 9 (all five
    # rounds), and not each other's
    assert got["A"].times["kernels_us"] == devpath._stats([4.0, 6.0, 8.0]) == {"median": 6.0, "p10": 4.4, "p90": 7.6}
    assert got["B"].times["kernels_us"] == devpath._stats([5.0, 7.0, 9.0]) == {"median": 7.0, "p10": 5.4, "p90": 8.6}
    assert got["A"].times["end_to_end_us"] == devpath._stats([104.0, 106.0, 108.0])
    assert got["B"].times["end_to_end_us"] == devpath._stats([105.0, 107.0, 109.0])
    assert list(got["A"].times) == ["kernels_us", "end_to_end_us", "python_us"]


def test_the_host_clock_is_read_immediately_round_each_call(monkeypatch):
    clock = [0.0]
    monkeypatch.setattr(devpath.time, "perf_counter", lambda: clock[0])
    # seconds each call of a step takes, round by round; only a step advances the clock, by exact binary fractions
    takes = {"A": iter([64.0, 1.0, 2.0, 4.0]), "B": iter([128.0, 8.0, 16.0, 32.0])}

    def step(name):
        def call():
            clock[0] += next(takes[name]) / 1024
            return result()
        return call
    got = devpath._timed("clock", {"A": step("A"), "B": step("B")}, reps=3, warmup=1)
    us = 1e6 / 1024
    # three kept values fix median, p10 and p90 and are fixed by them: the lists are exactly these, nothing of B in A's
    assert got["A"].host_us == got["A"].times["python_us"] == devpath._stats([1 * us, 2 * us, 4 * us])
    assert got["B"].host_us == devpath._stats([8 * us, 16 * us, 32 * us])
    assert got["A"].host_us["median"] == round(2 * us, 2) and got["B"].host_us["median"] == round(16 * us, 2)


def volumes(d2h_by_round):
    rounds = iter(d2h_by_round)
    return lambda: result(h2d_bytes=260, d2h_bytes=next(rounds))


def test_a_copy_volume_that_differs_in_a_kept_round_ends_the_command():
    steps = {"steady": volumes([500] * 5), "look_many": volumes([4096, 4096, 4096, 8192, 4096])}
    with pytest.raises(SystemExit) as e:
        devpath._timed("look 8, half", steps, reps=3, warmup=2)
    message = str(e.value)
    assert message.startswith("devpath: look 8, half: timed look_many calls copied")
    assert "(260, 4096)" in message and "(260, 8192)" in message and "500" not in message


def test_a_copy_volume_that_differs_in_the_warm_up_alone_is_no_error():
    steps = {"steady": volumes([500] * 5), "look_many": volumes([8192, 12288, 4096, 4096, 4096])}
    got = devpath._timed("look 8, half", steps, reps=3, warmup=2)
    assert got["look_many"].copied == {"h2d_bytes": 260, "d2h_bytes": 4096}
    assert got["steady"].copied == {"h2d_bytes": 260, "d2h_bytes": 500}
    assert got["look_many"].fields == {**got["look_many"].times, "h2d_bytes": 260, "d2h_bytes": 4096}


def test_a_timing_without_copy_fields_gives_times_and_no_copy_volume():
    got = devpath._timed("broadcast", {"broadcast": lambda: result(3.0, 5.0)}, reps=4, warmup=1)["broadcast"]
    assert got.copied == {} and list(got.fields) == ["kernels_us", "end_to_end_us", "python_us"]
    assert got.times["kernels_us"] == {"median": 3.0, "p10": 3.0, "p90": 3.0}
    assert got.times["end_to_end_us"] == {"median": 5.0, "p10": 5.0, "p90": 5.0}


def test_a_step_that_returns_nothing_gives_the_host_clock_alone():
    calls = []
    got = devpath._timed("cpu", {"look": lambda: result(h2d_bytes=1, d2h_bytes=2), "cpu": lambda: calls.append(0)},
                         reps=2, warmup=1)
    assert len(calls) == 3
    assert list(got["cpu"].times) == ["python_us"] and got["cpu"].copied == {}
    assert got["cpu"].host_us["median"] >= 0
    assert list(got["look"].times) == ["kernels_us", "end_to_end_us", "python_us"]


def test_one_kept_round_and_no_warm_up():
    calls = []

    def call():
        calls.append(0)
        return result(7.0, 9.0, h2d_bytes=3, d2h_bytes=4)
    got = devpath._timed("edge", {"only": call}, reps=1, warmup=0)["only"]
    assert len(calls) == 1
    assert got.times["kernels_us"] == {"median": 7.0, "p10": 7.0, "p90": 7.0}
    assert got.times["end_to_end_us"]["median"] == 9.0 and got.copied == {"h2d_bytes": 3, "d2h_bytes": 4}
