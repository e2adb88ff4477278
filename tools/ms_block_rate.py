#!/usr/bin/env python3
"""Frames per second of the multi-stream scorer's block call (s3a_ms_mgau_score_frames_dev: everything in HBM, 1024 frames in one
call) against a loop of s3a_ms_cont_mgau_frame_eval over the same frames -- the only way to do this work before the block call
existed -- on the hub4 ".s3cont." shape (synth.HUB4, top 4) and on a 256-density semi-continuous shape (1 codebook x 4 streams,
3000 senones).  One process: the two paths are checked against each other on the first 16 frames, warmed up, then timed in five
alternating repeats by a host clock around a device synchronise (a block repeat is 200 calls back to back, so that its window
is ~0.1 s).  For context (no threshold): the block call on the hub4 shape with top 8 beside s3a_mgau_score_frames_dev (.cont.) on
the same synthetic model.
usage (GPU box): python tools/ms_block_rate.py [out.json]      (default profiles/ms_block_rate.json); exits 2 without a GPU"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cmusphinx_amd import lib, synth

T, REPEATS, CHECK = 1024, 5, 16
BLOCK_CALLS = 200      # a timed block repeat = this many calls of T frames back to back (one call is ~0.5 ms: too short a window)


def shapes():
    m = synth.make_model(**synth.HUB4)
    hub4 = dict(mean=m["mean"], var=m["var"], mixw=m["mixw"], M=6144, nd=8, fl=[39], s2m=None,
                feats=synth.make_features(m, T, seed=9))
    rng = np.random.default_rng(3)
    fl, nd = [12, 24, 3, 12], 256
    D = sum(fl)
    semi = dict(mean=rng.standard_normal(nd * D).astype(np.float32),
                var=np.exp(rng.uniform(np.log(0.05), np.log(2.0), nd * D)).astype(np.float32),
                mixw=(rng.dirichlet(np.ones(nd) * 0.2, (3000, 4)) * 500).astype(np.float32), M=1, nd=nd, fl=fl,
                s2m=np.zeros(3000, np.int32), feats=(rng.standard_normal((T, D)) * 1.1).astype(np.float32))
    return hub4, semi


def sync():
    lib.check(lib.load().s3a_dev_sync())


def measure(a, topn, per_frame=True):
    ms = lib.MsMgau.init_arrays(a["mean"], a["var"], a["mixw"], a["M"], a["nd"], a["fl"], lib.LogMath(1.0003), topn,
                                sen2mgau=a["s2m"])
    S = ms.n_sen
    feats = np.ascontiguousarray(a["feats"], np.float32)
    fd = lib.DevBuf(feats.nbytes).upload(feats)
    sd = lib.DevBuf(T * S * 4)
    bd = lib.DevBuf(T * 4)
    ones = np.ones(S, np.uint8)
    row = np.zeros(S, np.int32)

    def block(calls=BLOCK_CALLS):
        t0 = time.perf_counter()
        for _ in range(calls):
            ms.score_frames_dev(fd, T, sd, best_dev=bd)
        sync()
        return calls * T / (time.perf_counter() - t0)

    def loop(n=T):
        t0 = time.perf_counter()
        for t in range(n):
            ms.frame_eval(ones, row, feats[t], t)
        return n / (time.perf_counter() - t0)

    # check: the two paths give the same rows and best
    block(1)
    rows, best = sd.download(np.int32, (T, S)), bd.download(np.int32, (T,))
    if per_frame:
        for t in range(CHECK):
            b = ms.frame_eval(ones, row, feats[t], t)
            if b != best[t] or not np.array_equal(row, rows[t]):
                raise SystemExit(f"block call and per-frame loop differ at frame {t}")
        loop(64)            # warm-up (block() ran above)
    block(8)
    res = {"block_frames_per_s": [], "per_frame_frames_per_s": []}
    for _ in range(REPEATS):
        res["block_frames_per_s"].append(round(block(), 1))
        if per_frame:
            res["per_frame_frames_per_s"].append(round(loop(), 1))
    return res


def measure_cont(a):
    """s3a_mgau_score_frames_dev (.cont.: every component, no top-N) on the same model and frames"""
    g = lib.MgauModel.init_arrays(a["mean"], a["var"], a["mixw"], lib.LogMath(1.0003))
    feats = np.ascontiguousarray(a["feats"], np.float32)
    fd = lib.DevBuf(feats.nbytes).upload(feats)
    sd = lib.DevBuf(T * g.S * 4)
    out = []
    for i in range(REPEATS + 1):
        t0 = time.perf_counter()
        for _ in range(BLOCK_CALLS):
            g.score_frames_dev(fd, T, sd)
        sync()
        if i:
            out.append(round(BLOCK_CALLS * T / (time.perf_counter() - t0), 1))
    return out


def main():
    lib.load()
    if lib.device_count() < 1:
        print("ms_block_rate: no HIP device", file=sys.stderr)
        return 2
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ms_block_rate.json")
    hub4, semi = shapes()
    res = {"frames": T, "repeats": REPEATS, "calls_per_block_repeat": BLOCK_CALLS,
           "timing": "host clock around a device synchronise; block = s3a_ms_mgau_score_frames_dev (device buffers), "
                     "per_frame = a loop of s3a_ms_cont_mgau_frame_eval (host buffers: its only form); alternating repeats, one process",
           "hub4_s3cont_top4": measure(hub4, 4), "semi256_top4": measure(semi, 4),
           "context_hub4_top8": {"block_frames_per_s": measure(hub4, 8, per_frame=False)["block_frames_per_s"],
                                 "cont_mgau_score_frames_dev_frames_per_s": measure_cont(hub4)}}
    ok = True
    for k in ("hub4_s3cont_top4", "semi256_top4"):
        r = res[k]
        r["slowest_block_over_fastest_per_frame"] = round(min(r["block_frames_per_s"]) / max(r["per_frame_frames_per_s"]), 2)
        ok = ok and r["slowest_block_over_fastest_per_frame"] > 1.0
    res["block_clears_per_frame_on_both_shapes"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
