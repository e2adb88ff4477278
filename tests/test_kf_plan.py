"""The host's plan of a ku_frames call (csrc/s3a_kfplan.h through s3a_kf_queue_plan: arithmetic on the utterances' lengths, runs without
a GPU): the order of the takes, the parts, the rows, the table of scoring groups in upload order and -- scoring beside the search -- the
second stream's script.

Two checks.  (1) The plan IS the one the code had before it was data: tests/golden/kf_plan_parent.json was recorded from that code's own
text (its two table writers, the cut / sort loops, the fix-up of the second piece's rows, the fill rules between the second stream's
launches) run on a stub.  (2) The plan is sound by its own properties, on the same inputs and on seeded random ones; among them a replay
of the script: no lane is ever told that a frame or an utterance is scored before the launch that scores it."""
import hashlib
import json
import os

import numpy as np
import pytest

from cmusphinx_amd import lib
from conftest import GOLDEN

FB, PIECE, I32MAX = 8, 1024, 2 ** 31 - 1
BUDGET, LANES, ONE = 0, 1, 2
SCORE, F_READY, Q_READY = 0, 1, 2
CASES = json.load(open(os.path.join(GOLDEN, "kf_plan_parent.json")))
IDS = [k for k, v in CASES.items() if isinstance(v, dict)]


def lengths_of(c):
    if "lengths" in c:
        return c["lengths"]
    g, x, out = c["lengths_gen"], c["lengths_gen"]["seed"], []
    for _ in range(g["n"]):
        x = (x * g["mul"] + g["add"]) % 2 ** 64
        out.append(g["lo"] + (x >> g["shift"]) % g["span"])
    return out


def plan_of(c):
    return lib.kf_queue_plan(lengths_of(c), c["rule"], c["budget"], c["in_order"], c["n1"], c["lead_groups"], c["round_groups"], c["whole"])


def test_the_fixture_is_the_issues_cases():
    assert IDS == list("abcdefghi") and len(CASES["parent"]) == 40
    a = CASES["a"]
    assert a["lengths"] == [40, 8, 9, 1, 64, 17, 17, 33, 7, 16, 25, 3] and (a["n1"], a["lead_groups"], a["round_groups"]) == (4, 1, 1)
    assert all(CASES[k]["lengths"] == a["lengths"] for k in "bcg") and CASES["b"]["whole"] and CASES["c"]["in_order"]
    assert CASES["d"]["lengths"] == [24] * 16 and len(CASES["f"]["cut"]) == 4 and CASES["g"]["rule"] == LANES
    assert CASES["e"]["f_ready0"] == I32MAX and CASES["h"]["rule"] == ONE and len(CASES["h"]["lengths"]) == 5
    n = lengths_of(CASES["i"])
    assert len(n) == 1024 and 300 <= min(n) and max(n) <= 2500 and (CASES["i"]["n1"], CASES["i"]["lead"], CASES["i"]["round_groups"]) == (256, 128, 4)


@pytest.mark.parametrize("case", IDS)
def test_plan_is_the_parents(case):
    c, p = CASES[case], plan_of(CASES[case])
    for k in ("max_rows", "g_first", "g_lead", "lead", "f_ready0"):
        assert p[k] == c[k], k
    assert p["n1"] == c["n1"]
    assert list(p["cut"]) == c["cut"] and list(p["g_at"]) == c["g_at"]
    for k in ("order", "row0", "groups", "steps"):
        flat = np.ascontiguousarray(p[k], "<i8").ravel()
        if k in c:
            assert flat.tolist() == c[k], k
        else:
            assert len(flat) == c[k + "_len"] and hashlib.sha256(flat.tobytes()).hexdigest() == c[k + "_sha256"], k


def check(n, rule, budget, in_order, n1, lead_g, round_g, whole, p):
    """the plan's own properties; n1, lead_g, round_g: as asked for"""
    n, N = np.asarray(n, np.int64), len(n)
    order, cut, row0, groups, steps = (p[k].tolist() for k in ("order", "cut", "row0", "groups", "steps"))
    parts = len(cut) - 1
    longest_first = lambda us: sorted(us, key=lambda u: -n[u])            # (sorted() is stable)
    # the parts and the takes
    assert cut[0] == 0 and cut[-1] == N and all(a < b for a, b in zip(cut, cut[1:]))
    if rule == BUDGET:
        for a, b in zip(cut, cut[1:]):          # consecutive utterances that fit, and the next one would not have
            assert n[a:b].sum() <= budget or b == a + 1
            assert b == N or n[a:b].sum() + n[b] > budget
            assert order[a:b] == (list(range(a, b)) if in_order else longest_first(range(a, b)))
    else:
        lanes = N if rule == ONE else budget
        assert cut == list(range(0, N, lanes)) + [N]
        assert order == (list(range(N)) if in_order or rule == ONE else longest_first(range(N)))
    assert sorted(order) == list(range(N))
    n1 = n1 if rule == BUDGET and parts == 1 and 0 < n1 < N else 0
    assert p["n1"] == n1
    # rows: from 0 in every part, one run without gaps -- along the takes, or (a plain queue's part scored up front) along the queue;
    # row0 by utterance for the queue's rule, by take for the others
    by_take = rule != BUDGET
    at = (lambda k: order[k]) if by_take or n1 > 0 else (lambda k: k)
    r0 = {}
    for a, b in zip(cut, cut[1:]):
        row = 0
        for k in range(a, b):
            assert row0[k if by_take else at(k)] == row
            r0[at(k)] = row
            row += int(n[at(k)])
        assert row <= p["max_rows"] and (rule != BUDGET or row <= budget or b == a + 1)
    assert p["max_rows"] == max(int(n[[at(k) for k in range(a, b)]].sum()) for a, b in zip(cut, cut[1:]))
    # the groups: every frame of every utterance in exactly one, in the utterance's part
    of = lambda u, a, b: [[u, f, min(FB, int(n[u]) - f), r0[u] + f] for f in range(a * FB, min(b * FB, int(n[u])), FB)]
    assert sorted(map(tuple, groups)) == sorted(tuple(g) for u in range(N) for g in of(u, 0, 1 << 40))
    assert all(f % FB == 0 and m == min(FB, n[u] - f) and r == r0[u] + f for u, f, m, r in groups)
    # ... in upload order
    n_g = lambda u: (int(n[u]) + FB - 1) // FB
    want, g_at = [], [0]
    if n1 == 0:
        for a, b in zip(cut, cut[1:]):
            want += [g for k in range(a, b) for g in of(at(k), 0, n_g(at(k)))]
            g_at.append(len(want))
        assert (p["g_first"], p["g_lead"], p["lead"], p["f_ready0"], steps) == (0, 0, 0, 0, [])
    else:
        top, a, rounds = max(n_g(order[k]) for k in range(n1)), 0, []
        while a < top and not whole:
            b = min(top, a + (lead_g if a == 0 else round_g))
            want += [g for k in range(n1) for g in of(order[k], a, b)]
            rounds.append((len(want), b * FB))
            a = b
        if whole:
            want += [g for k in range(n1) for g in of(order[k], 0, top)]
        assert p["g_first"] == len(want) == sum(n_g(order[k]) for k in range(n1))
        assert p["g_lead"] == (rounds[0][0] if rounds else len(want)) and p["lead"] == (rounds[0][1] if rounds else 0)
        want += [g for k in range(n1, N) for g in of(order[k], 0, n_g(order[k]))]
        g_at.append(len(want))
    assert groups == want and p["g_at"].tolist() == g_at
    if n1 == 0:
        return
    # the script, replayed
    scored, at_g, f_seq, q_seq = set(range(p["g_lead"])), p["g_lead"], [p["f_ready0"]] if p["lead"] else [], [n1]
    first_of = {}
    for i, g in enumerate(groups):
        first_of.setdefault(g[0], []).append(i)

    def frames_scored(u, lo, v):    # every group of u from frame lo on and below frame min(v, length) (what is below lo was checked)
        return all(i in scored for i in first_of[u][lo // FB:] if groups[i][1] < min(v, int(n[u])))

    assert all(frames_scored(u, 0, f_seq[0]) for u in order[:n1]) if f_seq else whole
    for op, a, b in steps:
        if op == SCORE:
            assert a == at_g and a < b <= a + PIECE and b <= len(groups)    # the launches cover the table once, in order
            scored.update(range(a, b))
            at_g = b
        elif op == F_READY:
            assert all(frames_scored(u, f_seq[-1], a) for u in order[:n1])
            f_seq.append(a)
        else:
            assert op == Q_READY
            lo = 0 if len(q_seq) == 1 else q_seq[-1]        # (the takes below the last value were checked then)
            assert all(i in scored for k in range(lo, a) for i in first_of[order[k]])
            q_seq.append(a)
    assert at_g == len(groups)
    assert all(x < y for x, y in zip(f_seq, f_seq[1:])) and all(x < y for x, y in zip(q_seq, q_seq[1:]))
    assert q_seq[-1] == N and (not f_seq or f_seq[-1] == I32MAX)


@pytest.mark.parametrize("case", IDS[:-1])
def test_plan_properties_of_the_recorded_cases(case):
    c = CASES[case]
    check(lengths_of(c), c["rule"], c["budget"], c["in_order"], c["n1"], c["lead_groups"], c["round_groups"], c["whole"], plan_of(c))


def test_plan_properties_of_the_bench_sized_case():
    c = CASES["i"]
    check(lengths_of(c), c["rule"], c["budget"], c["in_order"], c["n1"], c["lead_groups"], c["round_groups"], c["whole"], plan_of(c))


def test_plan_properties_random():
    for seed in range(300):
        rng = np.random.default_rng(seed)
        N = int(rng.integers(1, 60))
        n = rng.integers(1, int(rng.choice([9, 40, 300])), N)
        if seed % 7 == 0:
            n[:] = n[0]                                     # (equal lengths: the stable order)
        rule = int(rng.choice([BUDGET, BUDGET, LANES, ONE]))
        lanes = int(rng.integers(1, 20))
        budget = lanes if rule == LANES else 0 if rule == ONE else int(rng.choice([1 << 40, 1 << 40, n.sum() // 3 + 1, n.max()]))
        in_order, whole = bool(rng.integers(0, 2)) and rule != LANES, seed % 5 == 0
        n1, lead_g, round_g = int(rng.integers(0, N + 2)) * (seed % 3 != 0), int(rng.integers(1, 6)), int(rng.integers(1, 4))
        p = lib.kf_queue_plan(n, rule, budget, in_order, n1, lead_g, round_g, whole)
        check(n, rule, budget, in_order, n1, lead_g, round_g, whole, p)


def test_script_pieces_beyond_one_launch():
    """rounds and a tail of more than KFP_PIECE groups each: launches are split, and *q_ready follows piece by piece"""
    n = [400] * 60 + [24] * 200
    p = lib.kf_queue_plan(n, BUDGET, 1 << 40, False, 30, 2, 40, False)
    check(n, BUDGET, 1 << 40, False, 30, 2, 40, False, p)
    sc = [s for s in p["steps"].tolist() if s[0] == SCORE]
    assert max(b - a for _, a, b in sc) == PIECE and sum(1 for s in p["steps"].tolist() if s[0] == Q_READY) >= 2


def test_bad_arguments_are_refused():
    with pytest.raises(lib.S3AError):
        lib.kf_queue_plan([10, 0, 5], BUDGET, 100)
    with pytest.raises(lib.S3AError):
        lib.kf_queue_plan([10], 3, 100)
