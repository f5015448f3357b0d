"""How the GPU tier starts a child process, written once.

A ``test_device_*.py`` module runs its ``device_*_child.py`` once and asserts on the one tagged JSON line it prints; a
``test_devpath_*.py`` test runs ``python -m nuts333_amd.devpath`` and asserts on the one line that prints.  Both run
under ``timeout -k 10 <limit>`` with ``<limit> + 60`` seconds for ``subprocess`` on top, from the repository root, and a
child that does not finish, exits with anything but 0 or prints no result fails the test with its last 2000 bytes of stderr.
"""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent


def _run(what: str, limit: int, *argv: str) -> subprocess.CompletedProcess:
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, *argv]
    try:
        return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit + 60, cwd=str(REPO))
    except subprocess.TimeoutExpired:
        pytest.fail(f"{what} did not finish in {limit + 60} s")


def run_child(script: str, tag: str, limit: int, *args: str) -> dict:
    """``tests/<script> <args>``: the JSON of the last stdout line that starts with ``tag`` and a space."""
    p = _run("device child", limit, str(REPO / "tests" / script), *args)
    lines = [l for l in p.stdout.decode(errors="replace").splitlines() if l.startswith(tag + " ")]
    if p.returncode != 0 or not lines:
        pytest.fail(f"device child exited {p.returncode}: {p.stderr.decode(errors='replace')[-2000:]}")
    return json.loads(lines[-1][len(tag) + 1:])


def run_devpath_line(what: str, limit: int, *args: str) -> str:
    """``python -m nuts333_amd.devpath <args>``: its one stdout line; ``what`` names the run where it fails."""
    p = _run(what, limit, "-m", "nuts333_amd.devpath", *args)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    lines = p.stdout.decode().strip().splitlines()
    assert len(lines) == 1
    return lines[0]


def run_devpath(what: str, limit: int, *args: str) -> dict:
    """The JSON of ``run_devpath_line``."""
    return json.loads(run_devpath_line(what, limit, *args))
