"""The utterance engine's launch geometry (csrc/s3a_uttgeom.h through s3a_utt_geometry: arithmetic on the engine's shape, runs without a
GPU): the grids fixed at init, a frame's launches per lanes of a call, the scoring passes' shapes, ku_frames' cluster sizes, grids and
relay stages, the first lanes of a queue scored beside the search, and what a call runs as.

Two checks.  (1) The geometry IS the one the code had before it was data: tests/golden/utt_geometry_parent.json was recorded from that
code's own statements (the fixture names the commit and the functions) run on a stub, over three engine shapes crossed with the lane
counts, slots, options and variants the rules read; the retired options sit at their defaults.  (2) The geometry is sound by its own
properties, on the same inputs and on seeded random ones: no cluster grid beyond what an XCD holds, relay stages that shrink, scoring
passes that cover their slots within a CU's LDS, one route per call."""
import json
import os
import random

import pytest

from cmusphinx_amd import lib
from conftest import GOLDEN

FIX = json.load(open(os.path.join(GOLDEN, "utt_geometry_parent.json")))
SHAPES = list(FIX["shapes"])
LANES = [1, 7, 8, 9, 16, 17, 31, 32, 63, 64, 95, 96, 128, 255, 256, 257, 512, 1024]
TOTALS = [8, 16, 64, 1024, 4096, 8184]
KF_MAXC, KF_STAGES, CU_LDS, FB = 32, 2, 160 * 1024, 8
ROUTES = list(lib.GEOM_ROUTES)
CALL_FIELDS = ("queue", "n_utt", "alone", "prof_every", "second_pass", "keep_lat", "hist_sort_launch", "kf_no_relay", "kf_relay_at",
               "kf_no_overlap", "kf_overlap_n1", "kf_overlap_lead", "kf_overlap_round")


def rows(section):
    """the section's rows as (inputs dict, [output lists])"""
    sec = FIX["sections"][section]
    parts = [p.split() for p in sec["columns"].split("|")]
    for r in sec["rows"]:
        at, out = 0, []
        for p in parts:
            out.append(dict(zip(p, r[at:at + len(p)])) if not out else list(zip(p, r[at:at + len(p)])))
            at += len(p)
        assert at == len(r)
        yield out[0], out[1:]


def geometry(i, n, ov=0, score_slots=8, max_rows=0, budget=0):
    """inputs by name (the shape's id, shape fields, call fields) -> the hook's records"""
    shape = dict(FIX["shapes"][SHAPES[i["shape"]]])
    shape.update({k: v for k, v in i.items() if k in lib.geometry_fields("shape")})
    shape.setdefault("kf_slots", 512)
    shape.setdefault("kf_lds", 81376)
    call = {k: v for k, v in i.items() if k in CALL_FIELDS}
    return lib.utt_geometry(shape, call, n, ov, score_slots, max_rows, budget)


def same(record, want, what):
    got = [(k, record[k]) for k, _ in want]
    assert got == want, (what, got, want)


def test_the_fixture_is_the_issues_cases():
    assert FIX["parent"].startswith("dd02780") and "enqueue_frame" in FIX["copied_from"] and "kf_choose_c" in FIX["copied_from"]
    assert SHAPES == ["small", "hub4", "wide"]
    w = FIX["shapes"]["wide"]
    assert w["maxhmmpf"] >= 50000 and w["maxn"] >= 50000
    seen = {s: {c: set() for c in FIX["sections"][s]["columns"].split("|")[0].split()} for s in FIX["sections"]}
    for s in FIX["sections"]:
        for i, _ in rows(s):
            for k, v in i.items():
                seen[s][k].add(v)
    # (the cross product is trimmed to what each rule reads: the cluster and n1 rules read of the shape only what the row sets -- one shape;
    # the route reads it through n_emit / nodepk / the wide beam -- two; the lanes cross with the options where a rule compares them)
    assert seen["engine"]["shape"] == {0, 1, 2} == seen["frame"]["shape"] == seen["score"]["shape"]
    assert seen["kf"]["shape"] == {1} == seen["n1"]["shape"] and seen["route"]["shape"] == {0, 2}
    assert seen["engine"]["n_lanes"] == set(LANES) and seen["frame"]["n"] == set(LANES) and seen["kf"]["n"] == set(LANES)
    assert seen["route"]["n_utt"] == set(LANES) and seen["n1"]["n_lanes"] == set(LANES)
    assert seen["kf"]["kf_slots"] == {256, 512} and seen["kf"]["alone"] == {0, 1} and seen["kf"]["cluster"] == {0, 2, 3}
    assert seen["kf"]["kf_relay_at"] == {0, 4}
    assert seen["engine"]["persist"] == {-1, 0, 1, 2} == seen["route"]["persist"] and seen["engine"]["window"] == {-1, 0} == seen["route"]["window"]
    assert seen["route"]["pheurtype"] == {0, 1} == seen["n1"]["pheurtype"] and seen["route"]["second_pass"] == {0, 1} == seen["n1"]["second_pass"]
    assert seen["score"]["score_slots"] == set(TOTALS)


def test_engine_geometry_is_the_parents():
    for i, (want,) in rows("engine"):
        same(geometry(i, 1)["engine"], want, i)


def test_frame_geometry_is_the_parents():
    for i, (frame, window) in rows("frame"):
        g = geometry(i, i["n"])
        same(g["frame"], frame, i)
        same(g["window"], window, i)


def test_scoring_shapes_are_the_parents():
    for i, (score, comp) in rows("score"):
        g = geometry(dict(i, n_lanes=512), 1, score_slots=i["score_slots"])
        same(g["score"], score, i)
        same(g["companion"], comp, i)


def test_ku_frames_clusters_and_relay_are_the_parents():
    for i, (want,) in rows("kf"):
        same(geometry(i, i["n"], ov=i["ov"])["kf"], want, i)


def test_route_is_the_parents():
    for i, (want,) in rows("route"):
        n = min(i["n_lanes"], i["n_utt"]) if i["queue"] else i["n_utt"]
        g = geometry(i, n, max_rows=0 if i["fits"] else 1)
        assert [g["kf"]["served"], ROUTES.index(g["route"])] == [v for _, v in want], (i, g["kf"]["served"], g["route"], want)


def test_first_lanes_beside_the_search_are_the_parents():
    for i, (want,) in rows("n1"):
        same(geometry(dict(i, queue=1), i["n_lanes"])["kf"], want, i)


# ---- (2) properties ----
def fixture_inputs():
    """every fixture row as (inputs, n)"""
    for s in ("frame", "kf", "route", "n1"):
        for i, _ in rows(s):
            if s == "route":
                yield dict(i), (min(i["n_lanes"], i["n_utt"]) if i["queue"] else i["n_utt"])
            elif s == "n1":
                yield dict(i, queue=1), i["n_lanes"]
            else:
                yield dict(i), i["n"]


def random_inputs(count=400, seed=20261020):
    r = random.Random(seed)
    for _ in range(count):
        nl = r.choice(LANES + [2, 3, 40, 200, 300, 768])
        n = r.randint(1, nl)
        i = dict(shape=r.randrange(3), n_lanes=nl, kf_slots=r.choice([8, 64, 72, 256, 504, 512, 1024]), n_cu=r.choice([1, 8, 64, 256, 304]),
                 alone=r.randrange(2), cluster=r.choice([0, 0, 1, 2, 3, 8, 40]), kf_relay_at=r.choice([0, 0, 2, 4, 16]), kf_no_relay=r.randrange(4) == 0,
                 persist=r.choice([-1, 0, 0, 1, 2]), window=r.choice([-1, -1, 0, 8, 20]), pheurtype=r.randrange(2), second_pass=r.randrange(2),
                 keep_lat=r.randrange(4) == 0, queue=r.randrange(2), many=r.choice([0, 0, 2, 100]), scan_small_from=r.choice([0, 0, 2]),
                 big_wl=r.choice([-1, -1, 0, 1]), graph=r.randrange(8) == 0, framecheck=r.randrange(8) == 0, prof_every=r.choice([0, 0, 0, 4]),
                 kf_no_overlap=r.randrange(6) == 0, kf_overlap_n1=r.choice([0, 0, 0, 2, nl]), kf_overlap_lead=r.choice([0, 8, 20]),
                 kf_overlap_round=r.choice([0, 1, 3]), hist_sort_launch=r.randrange(2), kf_lds=r.choice([0, 40000, 81376, 81920, 120000]))
        i["n_utt"] = r.choice([n, nl, 2 * nl + 1]) if i["queue"] else n
        yield i, (min(nl, i["n_utt"]) if i["queue"] else n)


def check_kf(i, n, g):
    k, e = g["kf"], g["engine"]
    lanes_per_xcd = (n + 7) // 8
    for c, grid, m in ((k["C"], k["grid"], n), (k["c0"], k["grid0"], n)):
        assert 1 <= c <= KF_MAXC, (i, k)
        if c > 1:
            assert c * lanes_per_xcd <= k["usable"] and grid == 8 * c * lanes_per_xcd, (i, k)
        else:
            assert grid == m, (i, k)
    stages = [(k[f"st_c{j}"], k[f"st_cap{j}"], k[f"st_grid{j}"]) for j in (1, 2)][:k["n_st"]]
    assert 0 <= k["n_st"] <= KF_STAGES
    prev_c, prev_n = k["c0"], n
    if k["usable"] < 2:                 # (an XCD that holds no cluster of 2: no relay -- never a stage of no lanes, a launch of no workgroups)
        assert k["n_st"] == 0, (i, k)
    for c, cap, grid in stages:
        assert cap >= 1 and grid >= 8 * c, (i, k)
        assert c in (2, 4) and c > prev_c and cap < prev_n, (i, k)          # strictly growing clusters, falling caps
        assert cap * c // 8 <= k["usable"] and 5 * cap <= 4 * prev_n, (i, k)
        assert grid == 8 * c * ((cap + 7) // 8) and c * ((cap + 7) // 8) <= k["usable"], (i, k)
        prev_c, prev_n = c, cap
    # every condition kf_decode_queue's comment lists for n1 > 0
    if k["n1"] > 0:
        assert i.get("queue") and not i.get("kf_no_overlap") and not i.get("second_pass") and not i.get("pheurtype") and not i.get("keep_lat")
        assert i["n_utt"] > i["n_lanes"] and not i.get("cluster") and 0 < k["n1"] < i["n_lanes"], (i, k)
        if not i.get("kf_overlap_n1"):
            n_cu = max(1, i.get("n_cu", 256))
            assert i.get("alone") and n_cu < i["n_lanes"] <= 2 * n_cu + 1 and k["n1"] == i["n_lanes"] // 2, (i, k)
            assert geometry(i, i["n_lanes"])["kf"]["C"] == 1
        assert k["lead_g"] >= 1 and k["round_g"] >= 1
    # exactly one route; a ku_frames route implies that the call is served
    assert g["route"] in ROUTES
    if g["route"] in ("kf_static", "kf_queue", "kf_groups", "window"):
        assert k["served"] and e["persist"] > 0 and e["win_K"] > 0, (i, g["route"], k)
    if g["route"] == "graph":
        assert e["use_graph"] and e["persist"] == 0


def check_score(i, total, q, companion, room=None):
    assert q["fpc"] % FB == 0 and FB <= q["fpc"] <= 256 and q["n_chunks"] * q["fpc"] >= total, (i, total, q)
    assert q["lds"] <= CU_LDS and q["grid"] == (q["n_tiles"] + 7) // 8 * q["n_chunks"] * 8 and q["nt"] in (256, 512), (i, total, q)
    if companion:
        assert q["fpc"] <= 88 and q["nt"] == 256
        if q["tab_lds"]:
            assert q["lds"] <= room, (i, total, q, room)


def companion_room(kf_lds):
    lane = kf_lds if 0 < kf_lds <= CU_LDS // 2 else CU_LDS // 2
    return (CU_LDS - max((lane + 1279) // 1280 * 1280, (lane + 511) // 512 * 512)) // 1280 * 1280


@pytest.mark.parametrize("source", ["fixture", "random"])
def test_geometry_is_sound(source):
    count = 0
    for i, n in (fixture_inputs() if source == "fixture" else random_inputs()):
        for fits in (0, 1):
            g = geometry(i, n, ov=i.get("ov", 0), max_rows=1 - fits)
            check_kf(i, n, g)
        if g["engine"]["win_K"] > 0:
            check_score(i, n * g["engine"]["win_K"], g["window"], False)
        count += 1
    assert count >= 400


def test_scoring_passes_are_sound():
    r = random.Random(7)
    totals = TOTALS + [r.randint(1, 20000) for _ in range(200)]
    for s in range(3):
        for kf_lds in (0, 40000, 81368, 81376, 81920, 120000):
            for t in totals:
                i = dict(shape=s, n_lanes=512, kf_lds=kf_lds)
                g = geometry(i, 1, score_slots=t)
                check_score(i, t, g["score"], False)
                check_score(i, t, g["companion"], True, companion_room(kf_lds))
