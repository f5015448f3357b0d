"""Whole recorded sessions replayed, end to end, through the calls of ``device.Roster`` (tests/session_replay.py).

The twelve sessions tests/golden/reference_only/replay_<seed>.json are seeded random sessions recorded from the reference
build by tests/golden/make_replay_golden.py: four to six users of every level in several rooms, with clones, toggles and
invisible users between the speech; the last four also set rooms private and public, invite, ask to be let in, list the
rooms and set descriptions, topics and phrases.  One replayer keeps the whole talker's state and answers every line step
through the Roster's calls -- the read through ``input_many``, and what that hands back through the call of its command --;
every client's bytes, the actor's included, are compared whole with the recording at every step, and the two plans that
``relay_many`` and the call that composed it make of the same room line are compared with each other.

Host tier (unmarked): the CPU models of the per-call tests, joined by the replayer, reproduce all twelve sessions; the
sessions cover what they were chosen to cover; a model or a replayer that is wrong in one of nine known ways no longer
reproduces them; an unlisted command raises.  Where the reference build is present, every ``replay_*.json`` and ``who.json``
are recorded again and compared with the committed files.

GPU tier: ONE short-lived child for the module (tests/device_replay_child.py, under ``timeout``) replays the same sessions
on the device, each in two rosters that are seated once and keep their own state after that, and the tests assert on its
JSON: the bytes, the plans, the roster's host mirrors against the replayer's state after every step, and what the backend
uploaded after the logins.
"""
from __future__ import annotations

import copy
import json
import sys
from pathlib import Path

import pytest

import child_run
import device_clone_child
import device_go_child
import device_review_child
import device_tell_child
import scenarios
import session_replay
from nuts333_amd import device, nuts_path
from session_replay import COMPACT, COVERAGE, SEEDS, SPREAD, ReplayError, coverage_gaps, load, replay

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
CALLS = {"input_many", "relay_many", "tell_many", "look_many", "who_many", "review_many", "revtell_many", "go_many", "clone_many",
         "set_many", "access_many", "rooms_many"}


@pytest.fixture(scope="module")
def docs():
    return {seed: load(seed) for seed in SEEDS}


@pytest.fixture(scope="module")
def model_runs(docs):
    """Every session through the CPU models, in both layouts: computed once, read by the tests below."""
    return {(seed, layout): replay(doc, layout=layout) for seed, doc in docs.items() for layout in (COMPACT, SPREAD)}


# ------------------------------------------------------------------ host tier
def test_the_fixtures_are_small_sessions(docs):
    limit = (GOLDEN / "vectors" / "transducer.json").stat().st_size
    assert len(SEEDS) == len(set(SEEDS)) == 12 and SEEDS[:8] == session_replay.FIRST_SEEDS
    for seed, doc in docs.items():
        assert (GOLDEN / "reference_only" / f"replay_{seed}.json").stat().st_size < limit
        ops = [s["op"] for s in doc["steps"]]
        n = len(doc["accounts"][0])
        assert 4 <= n <= 6 and ops.count("login") == n and ops.count("line") == 60
        assert "line" not in ops[:2 * n]                                 # everybody logs in before the first line step
        assert doc["config"]["max_clones"] == 2
        assert not any(s.get("send", "").split()[:1] in ([".afk"], [".quit"], [".mode"], [".prompt"], [".charecho"]) for s in doc["steps"])


def test_the_models_reproduce_every_session(model_runs):
    for (seed, layout), res in model_runs.items():
        assert res["mismatches"] == [], (seed, layout, res["mismatches"][:2])
        assert res["plan_disagreements"] == 0 and res["plan_checks"] > 0
        assert res["answered"] == 60 and res["tracked"] == 0, (seed, res["answered"])
        n = len(res["slots"])                                           # every client at every step, the actor included
        assert res["comparisons"] >= n * 60
    for seed in SEEDS:                                                  # where the users sit changes nothing
        a, b = model_runs[seed, COMPACT], model_runs[seed, SPREAD]
        assert all(a[k] == b[k] for k in ("answered", "tracked", "comparisons", "plan_checks", "commands", "coverage"))
        assert a["slots"] == list(range(len(a["slots"]))) and a["capacity"] == 8 + 2 * len(a["slots"])
        assert set(b["slots"]) <= {0, 63, 64, 128, 255, 256} and b["capacity"] == 257 + 2 * len(b["slots"])
    spread = {s for seed in SEEDS for s in model_runs[seed, SPREAD]["slots"]}
    assert spread == {0, 63, 64, 128, 255, 256}
    assert session_replay.TRACKED == ()


def test_the_sessions_cover_what_they_were_chosen_for(docs, model_runs):
    assert coverage_gaps(docs) == []
    total = {k: sum(model_runs[seed, COMPACT]["coverage"][k] for seed in SEEDS) for k in COVERAGE}
    print("\n[replay] coverage", total)
    assert all(total.values()), total
    commands = {}
    for seed in SEEDS:
        for what, n in model_runs[seed, COMPACT]["commands"].items():
            commands[what] = commands.get(what, 0) + n
    print("[replay] commands", commands)
    assert set(commands) == {"say", "shout", "emote", "semote", "unknown", *session_replay.ANSWERED, *session_replay.TRACKED}


def test_the_settings_come_from_the_provisioned_config(docs):
    st = session_replay.State(docs[SEEDS[0]], COMPACT)
    assert (st.gatecrash, st.min_private, st.ignore_mp, st.max_clones) == (device_go_child.ARCH, 2, device_go_child.WIZ, 2)
    assert [rm["name"] for rm in st.rooms if rm["inlink"]] == [b"lounge"] and len(st.rooms) == 5


def test_an_unlisted_command_raises(docs):
    for send in (".afk", ".quit", ".prompt", ".bcast hello", ""):
        doc = copy.deepcopy(docs[SEEDS[0]])
        at = next(i for i, s in enumerate(doc["steps"]) if s["op"] == "line") + 5
        doc["steps"].insert(at, {"op": "line", "actor": "c", "send": send, "recv": {}})     # Carol is a WIZ: .bcast is hers
        with pytest.raises(ReplayError, match=f"step {at}"):
            replay(doc)


def _ignshout_ignored(monkeypatch):
    real = nuts_path.admits
    monkeypatch.setattr(nuts_path, "admits", lambda f, *rest: real([*f[:4], 0, f[5]], *rest))


def _substring_before_exact(monkeypatch):
    def get_user(users, word):
        name = device_tell_child.capitalised(word)
        order = [users[j] for j in sorted(users) if not users[j]["login"] and users[j]["name"]]
        return next((u["slot"] for u in order if name in u["name"]), None)
    monkeypatch.setattr(device_tell_child, "get_user", get_user)


def _record_cuts_at_199(monkeypatch):
    real = device_review_child.Rings.record
    monkeypatch.setattr(device_review_child.Rings, "record",
                        lambda self, rm, text: real(self, rm, text if len(text) < 199 else text[:199] + b"\n"))


def _nothing_hears_all(monkeypatch):
    real = session_replay.relays
    monkeypatch.setattr(session_replay, "relays", lambda records, *rest: real(
        [(o, r, session_replay.ALL if h == session_replay.NOTHING else h) for o, r, h in records], *rest))


def _go_ignores_the_links(monkeypatch):
    real = device_go_child.go
    monkeypatch.setattr(device_go_child, "go", lambda users, rooms, *rest: real(
        users, [{**rm, "links": list(range(len(rooms)))} for rm in rooms], *rest))


def _ignall_flips_before_its_line(monkeypatch):
    """The model of ``relay_many`` without its ``ignall=``: the line is relayed by the flag as ``set_call`` left it."""
    real = session_replay.ModelBackend.relay
    monkeypatch.setattr(session_replay.ModelBackend, "relay", lambda self, *a, ignall=None, **kw: real(self, *a, **kw))


def _clone_appears_as_a_presence(monkeypatch):
    real = device_clone_child.clone

    def clone(users, rooms, clones, slot, *rest):
        res = real(users, rooms, clones, slot, *rest)
        if res["outcome"] == device.CLONE_CREATED and not users[slot]["vis"]:
            res["there"] = res["there"].replace(users[slot]["name"], device.INVISNAME)
        return res
    monkeypatch.setattr(device_clone_child, "clone", clone)


def _destroyed_record_leaves_a_gap(monkeypatch):
    """The records as a table that is never compacted: a destroyed record stays empty until the next clone takes it."""
    real = device_clone_child.clone_call

    def clone_call(users, rooms, clones, events, *rest):
        before = list(clones)
        call = real(users, rooms, clones, events, *rest)
        res = call["events"][0]
        if res["outcome"] == device.CLONE_DESTROYED:
            clones[:] = before
            clones[res["record"]] = None
        elif res["outcome"] == device.CLONE_CREATED:
            new = clones[res["created"]]
            clones[:] = before
            clones[before.index(None)] = new
        return call
    monkeypatch.setattr(device_clone_child, "clone_call", clone_call)


def _invites_ignored(monkeypatch):
    real = device_go_child.has_room_access
    monkeypatch.setattr(device_go_child, "has_room_access", lambda u, *rest: real({**u, "invite": None}, *rest))


@pytest.mark.parametrize("mutate", [_ignshout_ignored, _substring_before_exact, _record_cuts_at_199, _nothing_hears_all,
                                    _go_ignores_the_links, _ignall_flips_before_its_line, _clone_appears_as_a_presence,
                                    _destroyed_record_leaves_a_gap, _invites_ignored])
def test_a_model_that_is_wrong_no_longer_reproduces_the_sessions(docs, monkeypatch, mutate):
    """The predicate ignores ignshout; get_user tries strstr before the exact pass; the ring cuts a line at 199 bytes; a clone
    told to hear nothing hears everything; a ``.go`` ignores the room's links, so every move walks; ``toggle_ignall`` flips
    the flag before its line goes out; ``.clone``'s there line names an invisible actor ``invisname``; a destroyed record
    leaves a gap instead of closing it; ``has_room_access`` ignores ``invite_room``: each of these is caught by the recorded
    bytes of some session."""
    mutate(monkeypatch)
    bad = {seed: len(replay(doc)["mismatches"]) for seed, doc in docs.items()}
    print("\n[replay]", mutate.__name__, bad)
    assert any(bad.values()), mutate.__name__


def test_keeping_everyone_in_room_0_no_longer_passes(docs):
    """What replay_reads of tests/device_input_child.py assumes -- nobody ever moves -- fails on every session but those
    in which nobody moved."""
    bad = {seed: len(replay(doc, everyone_in_room_0=True)["mismatches"]) for seed, doc in docs.items()}
    print("\n[replay] everyone in room 0", bad)
    assert sum(n > 0 for n in bad.values()) >= 6, bad


# ------------------------------------------------------------------ where the reference build is present
@pytest.mark.reference
@pytest.mark.parametrize("seed", SEEDS)
def test_a_session_regenerates_byte_for_byte(seed, ref_binary):
    import make_replay_golden
    again = make_replay_golden.render(make_replay_golden.record(seed, ref_binary))
    assert again == (GOLDEN / "reference_only" / f"replay_{seed}.json").read_text()


@pytest.mark.reference
def test_who_json_regenerates_byte_for_byte(ref_binary, monkeypatch):
    import make_who_golden
    monkeypatch.setitem(scenarios.REFERENCE_ONLY, "who", make_who_golden.who)
    again = json.dumps(make_who_golden.record(ref_binary), indent=1, ensure_ascii=True) + "\n"
    assert again == (GOLDEN / "reference_only" / "who.json").read_text()


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def replay_run(built):
    res = child_run.run_child("device_replay_child.py", "DEVICE_REPLAY", 300)
    print("\n[replay]", json.dumps(res)[:6000])
    return res


@pytest.mark.gpu
def test_the_device_reproduces_every_session_in_both_rosters(replay_run, model_runs):
    assert set(replay_run["sessions"]) == {f"{seed}/{layout}" for seed in SEEDS for layout in (COMPACT, SPREAD)}
    for (seed, layout), model in model_runs.items():
        got = replay_run["sessions"][f"{seed}/{layout}"]
        assert got["n_mismatches"] == 0, (seed, layout, got["mismatches"])
        for k in ("answered", "tracked", "comparisons", "plan_checks", "commands", "capacity", "slots"):
            assert got[k] == model[k], (seed, layout, k)
    assert replay_run["steps"] == 2 * 12 * 60


@pytest.mark.gpu
def test_input_many_and_relay_many_plan_the_same_line_alike(replay_run, model_runs):
    """Every room line a session speaks, and now the enter, leave, reset, here, there and said lines of the event calls
    too, against ``relay_many``'s plan of the same line: admit bitmap, both variants and chunk sizes of the two kernels' plans."""
    checks = sum(s["plan_checks"] for s in replay_run["sessions"].values())
    assert checks == sum(m["plan_checks"] for m in model_runs.values()) > 0
    assert all(s["plan_checks"] > 0 and s["plan_disagreements"] == 0 for s in replay_run["sessions"].values())


@pytest.mark.gpu
def test_every_call_of_the_roster_took_part(replay_run):
    for key, s in replay_run["sessions"].items():
        assert s["calls"]["input_many"] == 60 and s["calls"]["relay_many"] >= s["plan_checks"], key
    calls = {}
    for s in replay_run["sessions"].values():
        for what, n in s["calls"].items():
            calls[what] = calls.get(what, 0) + n
    assert set(calls) == CALLS
    assert all(n >= 16 for n in calls.values()), calls


@pytest.mark.gpu
def test_the_roster_kept_its_own_state(replay_run):
    """After the logins the backend uploaded the clones' look-seats and nothing else -- no user's slot, no room, no clone
    record --, and after every step the roster's host mirrors were what the replayer's state says: a mirror that differs is
    among the mismatches, which the first test of the tier found empty."""
    for key, s in replay_run["sessions"].items():
        assert s["mirror_checks"] == 60 and s["n_mismatches"] == 0, key
        assert not {int(slot) for slot in s["uploads"]["update"]} & set(s["slots"]), (key, s["uploads"])
        assert all(int(slot) > max(s["slots"]) for slot in s["uploads"]["update"]), (key, s["uploads"])
        assert s["uploads"]["set_clones"] == {} and s["uploads"]["set_rooms"] == {}, (key, s["uploads"])
    assert sum(len(s["uploads"]["update"]) for s in replay_run["sessions"].values()) > 0       # the look-seats were seated
