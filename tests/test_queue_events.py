"""The whole schedule of a queue call (csrc/s3a_qsched.h through s3a_queue_events: arithmetic on the utterances' lengths, runs without a
GPU): which lane decodes which utterance from which engine frame on under which scan epoch, what the lanes are left with, and the refill
events -- who ends, who begins -- as offsets into the flat lane / utterance lists that go to the device.

Two checks.  (1) The record IS what the code computed before it was data: tests/golden/queue_events_parent.json was recorded from that
code's own text (the schedule, the map of lists per boundary, the epoch hand-out, the groups' list loop) run on a stub.  (2) The record is
sound by its own properties, on the same inputs and on seeded random ones, by replaying the events: a wrong order here is what would
silently corrupt a lane."""
import hashlib
import json
import os

import numpy as np
import pytest

from cmusphinx_amd import lib
from conftest import GOLDEN
from test_kf_plan import lengths_of

LANES = 1           # kf_plan's rule of the second-pass queue
CASES = json.load(open(os.path.join(GOLDEN, "queue_events_parent.json")))
IDS = [k for k, v in CASES.items() if isinstance(v, dict)]
PER_UTT, PER_LANE = ("lane", "f0", "epoch"), ("last_utt", "epoch_after", "nfr_after")


def events_of(c):
    return lib.queue_events(c["n_lanes"], c["boundary"], lengths_of(c), c.get("epoch0"), c.get("groups", 0))


def test_the_fixture_is_the_issues_cases():
    A = [40, 8, 9, 1, 64, 17, 17, 33, 7, 16, 25, 3]
    assert IDS == list("abcdefghij")
    assert all(CASES[k]["lengths"] == A for k in "abcdgij")
    assert [(CASES[k]["n_lanes"], CASES[k]["boundary"]) for k in "abc"] == [(4, 8), (4, 1), (3, 16)]
    assert CASES["d"]["n_lanes"] == 40 and CASES["g"]["n_lanes"] == 1
    assert (CASES["e"]["lengths"], CASES["e"]["n_lanes"], CASES["e"]["boundary"]) == ([24] * 16, 4, 8)
    assert (CASES["f"]["lengths"], CASES["f"]["n_lanes"], CASES["f"]["boundary"]) == ([16, 17, 8, 9, 24, 1], 2, 8)
    n = lengths_of(CASES["h"])
    assert CASES["h"]["lengths_gen"] == json.load(open(os.path.join(GOLDEN, "kf_plan_parent.json")))["i"]["lengths_gen"]
    assert len(n) == 1024 and 300 <= min(n) and max(n) <= 2500 and (CASES["h"]["n_lanes"], CASES["h"]["boundary"]) == (256, 8)
    assert CASES["i"]["epoch0"] == [1, 500, 0, 77] and (CASES["i"]["n_lanes"], CASES["i"]["boundary"]) == (4, 8)
    assert CASES["j"]["groups"] == 1 and CASES["j"]["n_lanes"] == 8
    assert all("groups" not in CASES[k] and ("epoch0" in CASES[k]) == (k == "i") for k in "abcdefghi")


@pytest.mark.parametrize("case", IDS)
def test_record_is_the_parents(case):
    c, q = CASES[case], events_of(CASES[case])
    assert q["f_end"] == c["f_end"]
    for k in PER_UTT + PER_LANE + ("events", "lists"):
        flat = np.ascontiguousarray(q[k], "<i8").ravel()
        if k in c:
            assert flat.tolist() == c[k], k
        else:
            assert len(flat) == c[k + "_len"] and hashlib.sha256(flat.tobytes()).hexdigest() == c[k + "_sha256"], k


def check(n, n_lanes, boundary, epoch0, q):
    """the launch routes' record, its events replayed"""
    n, N, Z = [int(x) for x in n], len(n), min(n_lanes, len(n))
    lane, f0, epoch, last_utt, epoch_after, nfr_after, lists = (q[k].tolist() for k in PER_UTT + PER_LANE + ("lists",))
    assert all(len(a) == N for a in (lane, f0, epoch)) and all(len(a) == Z for a in (last_utt, epoch_after, nfr_after))
    sl, sf, total = lib.queue_schedule(n_lanes, boundary, n)
    assert lane == sl.tolist() and f0 == sf.tolist() and q["f_end"] == total
    running, used, begun, ended, at, last_f = {}, set(), [], [], 0, -1
    for f, o_end, o_beg, n_end, n_beg, max_nfr in q["events"].tolist():
        assert f > last_f and f % boundary == 0 and n_end + n_beg > 0                   # increasing frames, nothing empty
        last_f = f
        assert o_end == at and o_beg == o_end + 2 * n_end                               # the lists tile without gaps: ends, then begins
        at = o_beg + 2 * n_beg
        el, eu, bl, bu = lists[o_end:o_end + n_end], lists[o_end + n_end:o_beg], lists[o_beg:o_beg + n_beg], lists[o_beg + n_beg:at]
        assert eu == sorted(eu) and bu == sorted(bu)                                    # each in queue order
        for z, u in zip(el, eu):
            assert running.pop(z) == u                                                  # busy with exactly that utterance
            assert f == -(-(f0[u] + n[u]) // boundary) * boundary                       # ... which ends at the first boundary behind it
            ended.append(u)
        for z, u in zip(bl, bu):
            assert 0 <= z < Z and z not in running                                      # free: never used, or ended at this event or before
            assert lane[u] == z and f0[u] == f
            running[z] = u
            used.add(z)
            begun.append(u)
        assert max_nfr == max([n[u] for u in bu], default=0)
    assert at == len(lists) and not running and last_f == q["f_end"]                    # (the last event only ends lanes)
    assert sorted(begun) == sorted(ended) == list(range(N))                             # every utterance begins once and ends once
    e0 = [0] * Z if epoch0 is None else epoch0
    for z in range(Z):
        us = [u for u in range(N) if lane[u] == z]
        assert z in used and last_utt[z] == us[-1] and nfr_after[z] == n[us[-1]]
        assert epoch[us[0]] == max(e0[z], 1)
        # the stamps of a lane's consecutive utterances, [epoch, epoch + frames], never overlap
        assert all(epoch[a] + n[a] < epoch[b] for a, b in zip(us, us[1:])) and epoch[us[-1]] + n[us[-1]] < epoch_after[z]
        assert epoch_after[z] == max(e0[z], 1) + sum(n[u] + 1 for u in us)


@pytest.mark.parametrize("case", IDS[:-1])
def test_record_properties_of_the_recorded_cases(case):
    c = CASES[case]
    check(lengths_of(c), c["n_lanes"], c["boundary"], c.get("epoch0"), events_of(c))


def test_record_properties_random():
    for seed in range(300):
        rng = np.random.default_rng(seed)
        N, n_lanes, boundary = int(rng.integers(1, 80)), int(rng.integers(1, 24)), int(rng.choice([1, 8, 16, 64]))
        n = rng.integers(1, int(rng.choice([9, 40, 300])), N)
        if seed % 7 == 0:
            n[:] = boundary * int(rng.integers(1, 4))                                   # (every end coincides with a begin)
        epoch0 = None if seed % 3 == 0 else rng.integers(0, 1 << 20, min(n_lanes, N)).tolist()
        check(n, n_lanes, boundary, epoch0, lib.queue_events(n_lanes, boundary, n, epoch0))


def check_groups(n, n_lanes, q):
    """the form for groups of static launches: an event per part of the plan, lanes 0 .. m - 1 begin and end its takes"""
    n, N, Z = [int(x) for x in n], len(n), min(n_lanes, len(n))
    p = lib.kf_queue_plan(n, LANES, n_lanes)
    order, cut, lists, ev = p["order"].tolist(), p["cut"].tolist(), q["lists"].tolist(), q["events"].tolist()
    assert q["f_end"] == 0 and q["f0"].tolist() == [0] * N and q["epoch"].tolist() == [1] * N
    assert q["epoch_after"].tolist() == [1] * Z and q["nfr_after"].tolist() == [0] * Z
    assert len(ev) == len(cut) - 1
    want, last = [], [-1] * Z
    for (f, o_end, o_beg, n_end, n_beg, max_nfr), a, b in zip(ev, cut, cut[1:]):
        assert (f, o_end, o_beg, n_end, n_beg) == (0, len(want), len(want), b - a, b - a)
        assert max_nfr == max(n[u] for u in order[a:b]) == n[order[a]]                  # (longest first)
        want += list(range(b - a)) + order[a:b]
        for z, u in enumerate(order[a:b]):
            assert q["lane"][u] == z
            last[z] = u
    assert lists == want and q["last_utt"].tolist() == last


def test_groups_form_properties():
    c = CASES["j"]
    check_groups(c["lengths"], c["n_lanes"], events_of(c))
    for seed in range(100):
        rng = np.random.default_rng(seed)
        n, n_lanes = rng.integers(1, 300, int(rng.integers(1, 60))), int(rng.integers(1, 20))
        check_groups(n, n_lanes, lib.queue_events(n_lanes, 8, n, groups=True))


def test_bad_arguments_are_refused():
    for args in ((4, 8, [10, 0, 5]), (0, 8, [10]), (4, 0, [10]), (4, 8, [10, 5, 3, 2], [1, 2])):
        with pytest.raises(lib.S3AError):
            lib.queue_events(*args)
    with pytest.raises(lib.S3AError):
        lib.queue_events(4, 8, [10, 0], groups=True)
