"""A delivery plan for a resident roster: ``Roster.plan_many``, ``device.Plan`` and nuts_roster_plan of fanout.hip.

Host tier (unmarked): ``plan_many`` rejects what ``Roster.broadcast_many`` rejects, before the device library loads; the
arena bound does not apply to it and the variant bound does; a ``Plan`` built by hand from the CPU restatement alone
(``nuts_path.chunks`` / ``nuts_path.admits``), with gaps and garbage where the format allows them, expands into exactly
what ``expected()`` of tests/device_many_child.py gives.  The kernel's scratch-free compile is
tests/test_device_fanout.py's, over every name in ``device.KERNELS``.

GPU tier: everything that touches the device runs in ONE short-lived child for the module
(tests/device_plan_child.py, under ``timeout``), and the tests assert on its JSON: random calls and updates against the
restatement and against ``broadcast_many`` on the same roster, order independence, copy volume, the bench step and the
worst case.
"""
from __future__ import annotations

import json

import numpy as np
import pytest

import child_run
import test_device_roster as roster_tests
from device_many_child import Cpu, compare, expected
from nuts333_amd import device, nuts_path

FIELDS = ("admitted", "out_offsets", "arena", "write_offsets", "write_sizes", "broadcast_offsets")
GOOD = roster_tests.GOOD


def cases_of(test) -> list:
    """The argument values of a parametrised test of tests/test_device_roster.py."""
    return list(next(m for m in test.pytestmark if m.name == "parametrize").args[1])


# ------------------------------------------------------------------ host tier
@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the device library was loaded for input that must be rejected first")
    monkeypatch.setattr(device, "_load", refuse)


def test_the_plan_kernel_is_listed():
    assert "nuts_roster_plan" in device.KERNELS


MALFORMED = cases_of(roster_tests.test_broadcast_many_rejects_malformed_calls_before_the_device)
BAD_BROADCASTS = cases_of(roster_tests.test_broadcast_many_rejects_one_bad_broadcast_among_good_ones)


def test_the_malformed_calls_are_the_roster_tests_own():
    assert len(MALFORMED) == 8 and len(BAD_BROADCASTS) == 13


@pytest.mark.parametrize("call", MALFORMED)
def test_plan_many_rejects_malformed_calls_before_the_device(no_library, call):
    with pytest.raises(ValueError):
        roster_tests.roster().plan_many(call)


@pytest.mark.parametrize("bad", BAD_BROADCASTS)
def test_plan_many_rejects_one_bad_broadcast_among_good_ones(no_library, bad):
    with pytest.raises(ValueError, match=r"^broadcast 1: "):
        roster_tests.roster().plan_many([GOOD, bad, GOOD])
    with pytest.raises(ValueError) as plan_error:
        roster_tests.roster()._prepare_plan([GOOD, bad, GOOD])
    with pytest.raises(ValueError) as fanout_error:
        roster_tests.roster()._prepare([GOOD, bad, GOOD])
    assert str(plan_error.value) == str(fanout_error.value)             # the same rules, the same messages


def test_a_closed_roster_raises(no_library):
    with roster_tests.roster() as r:
        pass
    with pytest.raises(ValueError, match="closed"):
        r.plan_many([GOOD])


def test_prepare_plan_packs_what_prepare_packs(no_library):
    r = roster_tests.roster()
    calls = [(b"ab\n", 3, 7, 1, device.COM_SHOUT), ("", None, None, 0, device.COM_SAY),
             (b"xyz", 0, 0, True, device.COM_SEMOTE)]
    for got, want in zip(r._prepare_plan(calls), r._prepare(calls)):
        assert type(got) is type(want)
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and got.tolist() == want.tolist()
        else:
            assert got == want


def test_the_arena_bound_does_not_apply_and_the_variant_bound_does(no_library, monkeypatch):
    text = b"\n" * 1999
    per = device.max_bytes(len(text))
    r = device.Roster(device.MAX_CAPACITY)
    r.update(range(device.MAX_CAPACITY), room=0)
    k = device.MANY_ARENA_CAP // (device.MAX_CAPACITY * per)
    call = [(text, 0, None, 0, device.COM_SAY)] * (k + 1)
    with pytest.raises(ValueError, match="MANY_ARENA_CAP"):
        r._prepare(call)                                                # broadcast_many refuses it: slots x bytes
    packed = r._prepare_plan(call)                                      # there is no arena: it is planned
    assert len(packed[0]) == (k + 1) * 1999 and packed[2].tolist() == [1999] * (k + 1)
    # the variant bound, 12 * text bytes + 16 * K, at a lowered cap (the check reads the attribute when called)
    monkeypatch.setattr(device, "MANY_ARENA_CAP", 100_000)
    most = (100_000 - 16 * 5) // 12                                     # text bytes five broadcasts may sum to
    lens = [1999, 1999, 1999, 1999, most - 4 * 1999]
    r._prepare_plan([(b"x" * n, 0, None, 0, device.COM_SAY) for n in lens])
    lens[-1] += 1
    with pytest.raises(ValueError, match=r"variant bound.*MANY_ARENA_CAP"):
        r._prepare_plan([(b"x" * n, 0, None, 0, device.COM_SAY) for n in lens])
    with pytest.raises(ValueError, match=r"variant bound.*MANY_ARENA_CAP"):
        r.plan_many([(b"x" * n, 0, None, 0, device.COM_SAY) for n in lens])


def test_k_times_bitmap_words_stays_below_2_to_the_31(no_library):
    r = device.Roster(64)                                               # one word per broadcast
    with pytest.raises(ValueError, match="2\\^31"):
        r._prepare_plan(_Repeated(GOOD, 2**31))
    big = device.Roster(device.MAX_CAPACITY)
    big._prepare_plan([GOOD] * (1 << 15))                               # K x capacity = 2^31, K x W = 2^25: planned
    with pytest.raises(ValueError, match="2\\^31"):
        big._prepare([GOOD] * (1 << 15))


class _Repeated:
    """A sequence of ``n`` times one item that does not hold them (the size check comes before any item is read)."""

    def __init__(self, item, n):
        self.item, self.n = item, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not 0 <= i < self.n:
            raise IndexError(i)
        return self.item


# ---------------------------------------------- a Plan built by hand from the restatement
TEXTS = (b"", b"\n" * 1999, b"~OLUaaa shouts:~RS hello /~FR there\n", b"plain\n", b"~FRred~RS\n" * 20, b"nobody\n")
CAPACITIES = (1, 63, 64, 65, 256, 257, 1000)


def hand_built(capacity: int, seed: int = 5):
    """A roster of random slots (host only), six broadcasts to it -- the last one to a room nobody is in -- and their
    Plan from the CPU restatement alone: variants at scattered places of a buffer of 0xAA bytes, unused chunk sizes
    -7.  Returns the plan, the calls as broadcast_many tuples over roster.table(), and the listener records."""
    rng = np.random.default_rng(seed + capacity)
    r = device.Roster(capacity)
    r.update(range(capacity), room=[None if x == 3 else int(x) for x in rng.integers(0, 4, capacity)],
             login=(rng.random(capacity) < 0.1).tolist(), ignall=rng.integers(0, 2, capacity).tolist(),
             ignshout=rng.integers(0, 2, capacity).tolist(), colour=rng.integers(0, 2, capacity).tolist())
    calls = [(TEXTS[0], None, None, 1, device.COM_SAY), (TEXTS[1], 0, None, 0, device.COM_SAY),
             (TEXTS[2], None, int(rng.integers(capacity)), 0, device.COM_SHOUT),
             (TEXTS[3], 1, int(rng.integers(capacity)), 1, device.COM_SEMOTE),
             (TEXTS[4], 2, None, 0, device.COM_SHOUT), (TEXTS[5], 77, None, 1, device.COM_SAY)]
    k, words = len(calls), (capacity + 63) // 64
    bits = np.zeros((k, words), dtype=np.uint64)
    variants = np.full(60_000, 0xAA, dtype=np.uint8)
    starts, sizes = np.zeros((k, 2), dtype=np.int64), np.zeros((k, 2), dtype=np.int64)
    counts = np.zeros((k, 2), dtype=np.int32)
    wsz = np.full((k, 2, device.MAX_WRITES), -7, dtype=np.int32)
    at = 13
    as_tables, records = [], []
    for b, (text, rm, sender, force_listen, com) in enumerate(calls):
        table = r.table(rm, sender)
        admitted = np.array([nuts_path.admits(row[:6], rm is None, force_listen, com) for row in table.tolist()])
        padded = np.zeros(words * 64, dtype=bool)
        padded[:capacity] = admitted
        bits[b] = np.packbits(padded, bitorder="little").view(np.uint64)
        for c in (1, 0):                                                # colour-on first: the order is not fixed either
            ch = nuts_path.chunks(text, c)
            data = b"".join(ch)
            starts[b, c], sizes[b, c], counts[b, c] = at, len(data), len(ch)
            variants[at:at + len(data)] = np.frombuffer(data, dtype=np.uint8)
            wsz[b, c, :len(ch)] = [len(x) for x in ch]
            at += len(data) + 1 + 7 * b                                 # a gap of garbage after every variant
        as_tables.append((text, table, int(rm is None), force_listen, com))
        records.append((table.astype(np.int64) << np.arange(7)).sum(axis=1))
    colour = np.zeros(words * 64, dtype=bool)
    colour[:capacity] = r.table(None, None)[:, device.LISTENER_FIELDS.index("colour")] != 0
    plan = device.Plan(capacity=capacity, admitted_bits=bits,
                       colour_bits=np.packbits(colour, bitorder="little").view(np.uint64), variants=variants,
                       variant_starts=starts, variant_sizes=sizes, write_counts=counts, write_sizes=wsz, timing={})
    r.close()
    return plan, as_tables, records


@pytest.mark.parametrize("capacity", CAPACITIES)
def test_a_hand_built_plan_expands_into_the_restatements_fanout(no_library, capacity):
    plan, as_tables, records = hand_built(capacity)
    r = plan.expand()
    want = expected(Cpu(), as_tables, records)
    bad, first = compare(r, want, as_tables)
    assert bad == 0, first
    assert r.admitted.dtype == np.bool_ and r.out_offsets.dtype == np.int64 and r.write_offsets.dtype == np.int64
    assert r.arena.dtype == np.uint8 and r.write_sizes.dtype == np.int32
    assert r.broadcast_offsets.tolist() == [capacity * b for b in range(len(as_tables) + 1)]
    assert len(r.admitted) == capacity * len(as_tables) and len(r.arena) == r.out_offsets[-1]
    assert r.item(2, capacity - 1) == 3 * capacity - 1
    if capacity >= 63:                                                  # the random slots cover these
        assert plan.admitted(1).any() and plan.admitted(2).any() and not plan.admitted(1).all()
    assert not plan.admitted(5).any()                                   # a room nobody is in
    lo, hi = capacity * 5, capacity * 6
    assert r.out_offsets[lo] == r.out_offsets[hi] and r.write_offsets[lo] == r.write_offsets[hi]


@pytest.mark.parametrize("capacity", CAPACITIES)
def test_recipients_split_the_admitted_slots_by_colour(no_library, capacity):
    plan, as_tables, _ = hand_built(capacity)
    colour = as_tables[0][1][:, device.LISTENER_FIELDS.index("colour")]
    for b in range(len(as_tables)):
        admitted = plan.admitted(b)
        assert admitted.dtype == np.bool_ and admitted.shape == (capacity,)
        off, on = plan.recipients(b, 0), plan.recipients(b, 1)
        assert np.issubdtype(off.dtype, np.integer) and np.issubdtype(on.dtype, np.integer)
        assert (np.diff(off) > 0).all() and (np.diff(on) > 0).all()
        assert not set(off.tolist()) & set(on.tolist())
        assert sorted(off.tolist() + on.tolist()) == np.flatnonzero(admitted).tolist()
        assert (colour[off] == 0).all() and (colour[on] == 1).all()


def test_variants_and_chunks_are_the_restatements(no_library):
    plan, as_tables, _ = hand_built(65)
    for b, (text, *_) in enumerate(as_tables):
        for c in (0, 1):
            assert plan.chunks(b, c) == nuts_path.chunks(text, c)
            assert plan.variant(b, c) == nuts_path.transduce(text, c)
    # an empty text: nothing with colour off, the 4-byte reset in one write with colour on
    assert plan.variant(0, 0) == b"" and plan.chunks(0, 0) == [] and plan.write_counts[0].tolist() == [0, 1]
    assert plan.chunks(0, 1) == [b"\x1b[0m"]
    # 1999 newlines: 3,998 bytes in 5 writes, 11,998 bytes in 14 writes
    assert plan.variant_sizes[1].tolist() == [3998, 11_998] and plan.write_counts[1].tolist() == [5, 14]
    assert [len(x) for x in plan.chunks(1, 1)] == plan.write_sizes[1, 1, :14].tolist()
    for k, c in ((6, 0), (-1, 0), (0, 2)):
        with pytest.raises(IndexError):
            plan.variant(k, c)


def test_expand_needs_nothing_but_the_plans_own_arrays(no_library):
    plan, as_tables, records = hand_built(257)
    first = plan.expand()
    keep = {f: np.copy(getattr(plan, f)) for f in ("admitted_bits", "colour_bits", "variants", "variant_starts",
                                                   "variant_sizes", "write_counts", "write_sizes")}
    again = plan.expand()
    assert all(np.array_equal(getattr(first, f), getattr(again, f)) for f in FIELDS)
    assert all(np.array_equal(getattr(plan, f), v) for f, v in keep.items())       # expand() changes nothing
    # one admit bit more, on a slot that had none: exactly that item appears
    b, free = 3, int(np.flatnonzero(~plan.admitted(3))[0])
    plan.admitted_bits[b, free // 64] |= np.uint64(1) << np.uint64(free % 64)
    more = plan.expand()
    i = more.item(b, free)
    c = int(as_tables[0][1][free, device.LISTENER_FIELDS.index("colour")])
    assert more.admitted.sum() == first.admitted.sum() + 1 and more.output(i) == plan.variant(b, c)
    assert device.chunks(more, i) == plan.chunks(b, c)


# ------------------------------------------------------------------ GPU tier: one child for the module
@pytest.fixture(scope="module")
def plan_run(built):
    res = child_run.run_child("device_plan_child.py", "DEVICE_PLAN", 900)
    print("\n[plan]", json.dumps(res)[:1500])
    return res


@pytest.mark.gpu
def test_random_calls_and_updates_match_the_restatement_and_broadcast_many(plan_run):
    r = plan_run["random"]
    assert sorted(set(r["capacities"])) == [1, 2, 255, 256, 257, 1000, 1015, 4096]
    assert set(r["ks"]) >= {1, 7, 100, 1000} and r["calls"] >= 32 and r["items"] >= 1_000_000
    assert r["calls_without_update"] > 0 and r["updates"] > 0
    assert r["records_seen"] == 96 and r["rm_forms"] == ["every room", "room"]
    assert r["sender_forms"] == ["none", "slot"]
    assert r["n_bad_plan"] == 0, r["first_bad_plan"]                   # bits, variants, chunk sizes, tails, colour bits
    assert r["n_bad_expand"] == 0, r["first_bad_expand"]               # expand() == broadcast_many, all six fields


@pytest.mark.gpu
def test_plans_and_fanouts_mix_in_any_order_on_one_roster(plan_run):
    o = plan_run["order"]
    assert o["n_bad"] == 0, o
    assert o["steps"] == ["plan_many", "broadcast_many", "update", "broadcast_many", "plan_many"]
    assert o["update_changed_the_result"] is True
    assert o["earlier_plan_unchanged"] is True
    assert o["two_rosters_alternately_identical"] is True and o["two_rosters_differ"] is True


@pytest.mark.gpu
def test_copy_volume_is_fixed_by_the_shapes(plan_run):
    h = plan_run["copies"]["h2d"]
    assert h["clean"]["256"] == h["clean"]["4096"] > 0                  # no table travels
    for cap in ("256", "4096"):
        assert h["dirty"][cap] - h["clean"][cap] == 5 * int(cap), h
        assert h["after_update"][cap] == h["dirty"][cap] and h["clean_again"][cap] == h["clean"][cap], h
    d = plan_run["copies"]["d2h"]
    assert d["admitted_everyone"] == d["capacity"] * d["k"] and d["admitted_nobody"] == 0
    assert d["everyone"] == d["nobody"] > 0                             # not a function of who is admitted
    k, words = d["k"], (d["capacity"] + 63) // 64
    bound = (12 * d["text_bytes"] + 16 * k + 8 * k * words + 2 * k * (8 + 4 + 4 * device.MAX_WRITES) + 4 + 8 * 256)
    assert d["everyone"] <= bound, (d, bound)


@pytest.mark.gpu
def test_bench_step_of_100_shouts_to_a_1000_slot_roster(plan_run):
    b = plan_run["bench_step"]
    assert b["broadcasts"] == 100 and b["deliveries"] == 99_900          # counted from the bits
    assert b["n_bad"] == 0, b["first_bad"]
    t = b["timing"]
    assert 0 < t["kernels_us"] <= t["end_to_end_us"] and t["h2d_bytes"] > 0
    assert 0 < t["d2h_bytes"] < b["fanout_d2h_bytes"] / 20, (t, b["fanout_d2h_bytes"])


@pytest.mark.gpu
def test_worst_case_variants_and_buffer_reuse(plan_run):
    w = plan_run["worst"]
    assert w["broadcasts"] == 64 and w["deliveries"] == 64 * 64
    assert w["variant_pairs"] == [[[3998, 5], [11_998, 14]]]
    assert w["cpu_pair"] == [[3998, 5], [11_998, 14]]                   # as nuts_path.chunks gives them
    assert w["n_bad"] == 0, w["first_bad"]
    assert w["reuse_identical"] is True
