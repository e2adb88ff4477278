"""The launch geometry a LIVE engine holds (s3a_uttdec_geometry) is the pure function's (s3a_utt_geometry, csrc/s3a_uttgeom.h) on the shape
the engine reports -- the records tests/test_utt_geometry.py checks without a GPU are the ones the launches are made from --, and a call
runs with the cluster size its record names.  Four engines on the tidigits bundle: ku_frames forced with clusters of 2, the defaults, the
many-lane grids and 256-thread kernels forced onto a handful of lanes, the wide-beam word level forced."""
import pytest

import test_gpu_queue as TQ
from cmusphinx_amd import bundle, lib
from test_gpu_uttdec import tidigits_bundle  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ENGINES = {
    "3 lanes, ku_frames, clusters of 2": (3, {"persist": 1, "cluster": 2}, {}),
    "8 lanes": (8, {}, {}),
    "40 lanes, many-lane kernels": (40, {}, {"S3A_UTT_MANY": "2", "S3A_UTT_SCAN_SMALL": "2"}),
    "3 lanes, wide-beam word level": (3, {}, {"S3A_UTT_BIGWL": "1"}),
}


def pure(g, n):
    """the pure functions on what the engine reports (the window's scoring pass: the hook's `window` record)"""
    p = lib.utt_geometry(g["shape"], g["call"], n, ov=0)
    return {k: p[k] for k in ("engine", "frame", "window", "kf")}, p["route"]


def test_the_lookahead_switched_on_and_off_again(gpu_lib, tidigits_bundle):
    """s3a_uttdec_enable_pheur switches -pheurtype on and, with 0, off: the shape's copy follows at the next call, the route goes from the
    plain queue to groups of static launches and back, and ku_frames' occupancy and static LDS are asked again of the instantiation that
    is launched (the HEUR one, then the plain one again) -- after which the queue decodes as an engine that never had the look-ahead"""
    import numpy as np
    dec = bundle.Decoder(tidigits_bundle, 3, opts={"persist": 1})
    utts, feats = TQ.tidigits_feats(gpu_lib)
    rm, rs = TQ.ref_lines()

    def run():
        dec.decode_queue(feats[:7])
        g = dec.ud.geometry(3)
        return g, pure(g, 3)[1]
    g0, route0 = run()
    assert g0["shape"]["pheurtype"] == 0 and route0 == "kf_queue" and g0["shape"]["kf_slots"] > 0 and g0["shape"]["kf_lds"] > 0
    assert TQ.queue_lines(dec, utts[:7]) == (rm[:7], rs[:7])
    b = dec.b
    on = (1, -2000000, 1, [np.asarray(t["ci"], np.int32).astype(np.uint8) for t in b["trees"]],
          np.asarray(b["sen2cimap"], np.int32)[:b["n_ci_sen"] + 1].astype(np.int16), b["n_ci"])
    dec.ud.enable_pheur(*on)
    g1, route1 = run()
    assert g1["shape"]["pheurtype"] == 1 and route1 == "kf_groups" and g1["shape"]["kf_slots"] > 0 and g1["shape"]["kf_lds"] > 0
    dec.ud.enable_pheur(0, *on[1:])
    g2, route2 = run()
    assert g2["shape"] == g0["shape"] and route2 == "kf_queue" and g2["kf"] == g0["kf"]
    assert TQ.queue_lines(dec, utts[:7]) == (rm[:7], rs[:7])
    assert dec.ud.last_parts()["n_frames"] == 1            # (KF_QUEUE: one chain for the queue, not a launch per group)


@pytest.mark.parametrize("name", list(ENGINES))
def test_the_engine_launches_from_the_pure_functions_records(gpu_lib, tidigits_bundle, monkeypatch, name):
    n_lanes, opts, env = ENGINES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dec = bundle.Decoder(tidigits_bundle, n_lanes, opts=opts)
    g = dec.ud.geometry(n_lanes)
    assert g["shape"]["n_lanes"] == n_lanes and g["shape"]["T"] >= 2 and g["shape"]["N"] > 0 and g["shape"]["gp_n"] > 0
    assert {k: g[k] for k in ("engine", "frame", "window", "kf")} == pure(g, n_lanes)[0]
    if "S3A_UTT_MANY" in env:
        assert g["engine"]["many"] == 2 and g["engine"]["scan_small_from"] == 2
    if "S3A_UTT_BIGWL" in env:
        assert g["engine"]["big_wl"] == 1 and g["frame"]["g_wide"] > 0 and not g["frame"]["by_parents"]
    utts, feats = TQ.tidigits_feats(gpu_lib)
    dec.decode_queue(feats[:3])
    m, s = TQ.queue_lines(dec, utts[:3])
    rm, rs = TQ.ref_lines()
    assert m == rm[:3] and s == rs[:3]
    g = dec.ud.geometry(3)              # (now with the call's facts, and ku_frames' occupancy and LDS where the engine may run it)
    records, route = pure(g, 3)
    assert {k: g[k] for k in records} == records
    assert g["call"]["queue"] == 1 and g["call"]["n_utt"] == 3
    if g["engine"]["persist"]:
        assert g["shape"]["kf_slots"] >= g["shape"]["n_cu"] > 0 and g["shape"]["kf_lds"] > 0
    kf_route = route in ("kf_static", "kf_queue", "kf_groups", "window")
    assert kf_route == ("persist" in opts)
    if "S3A_UTT_MANY" in env:
        assert g["frame"]["by_parents"] and g["frame"]["enter2_threads"] == 256 and g["frame"]["scan_threads"] == 256
    assert dec.ud.last_parts()["cluster"] == (g["kf"]["c0"] if kf_route else 0)
    if "cluster" in opts:
        assert g["kf"]["c0"] == g["kf"]["C"] == opts["cluster"]
