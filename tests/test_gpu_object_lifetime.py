"""Device objects that live, grow and die several times in one process (MI355X).  Every object of cmusphinx_amd/csrc/ allocates its device
and pinned memory through one owner (s3a_hostmem.h) and its free function ends in that owner's free_all(); what an object borrows -- a
lextree clone's static arrays, a scorer's Gaussian-selection state when it is the model's -- its owner never hears of.

pocketsphinx engine: ONE engine of 2 lanes takes queues of 3, then 9, then 2 utterances (ref_ps_amdfwd -queue makes one call per process:
no other test reuses an engine's staging and queue buffers, grows them, and then uses them smaller than they are).  Every hypothesis must
be the one a fresh engine gives for that one call, and the 2-utterance call also s3a_psfwd_decode's on a fresh engine.

Lextree search (prototype + two clones), scorer (the model's state / its own) and multi-stream scorer: created, used and freed three
times; every life gives what the existing test of that object asserts (the helpers and goldens are those tests'), and the same as the
other lives."""
import ctypes as C

import numpy as np
import pytest

import lextree_trace
import psfwd_synth as PS
from conftest import golden
from test_gpu_frame_eval import tid  # noqa: F401  (fixture)
from test_gpu_lextree import load as load_lextree_trace, make_gpu

pytestmark = pytest.mark.gpu
N_SEN, N_DENSITY, VECLEN, TOPN = 160, 8, 39, 4
CALLS = [3, 9, 2]               # utterances per call, on one engine


def make_scorer(gpu_lib, seed):
    """-> (PsMsMgau over N_SEN continuous senones, its means [N_SEN][N_DENSITY][VECLEN])"""
    r = np.random.default_rng(seed)
    mean = r.standard_normal((N_SEN, N_DENSITY, VECLEN)).astype(np.float32)
    var = r.uniform(0.5, 2.0, (N_SEN, N_DENSITY, VECLEN)).astype(np.float32)
    mixw = r.dirichlet(np.ones(N_DENSITY), N_SEN).astype(np.float32)
    return gpu_lib.PsMsMgau.init_arrays(mean, var, mixw, N_SEN, N_DENSITY, [VECLEN], TOPN), mean


def make_utts(seed, mean, pl_window):
    """sum(CALLS) utterances of 20..60 frames, no two of one call equally long; a frame = some Gaussian's mean + noise"""
    r = np.random.default_rng(seed)
    utts = []
    for n in CALLS:
        lens = r.choice(np.arange(20, 61), n, replace=False)
        assert lens.min() > pl_window and len(set(lens)) == n
        for ln in lens:
            s, d = r.integers(0, N_SEN, ln), r.integers(0, N_DENSITY, ln)
            utts.append(np.ascontiguousarray(mean[s, d] + 0.3 * r.standard_normal((ln, VECLEN)), np.float32))
    return utts


def call_args(feats):
    ptrs = (C.c_void_p * len(feats))(*[f.ctypes.data for f in feats])
    nfr = np.array([len(f) for f in feats], np.int32)
    return C.cast(ptrs, C.c_void_p), nfr        # (the cast keeps ptrs alive)


def decode_queue(dev, ps, feats):
    """s3a_psfwd_decode_queue + every s3a_psfwd_queue_hyp -> [(score, [(wid, sf, ef, ascr, lscr, bp)])], as Device.hyp gives them"""
    ptrs, nfr = call_args(feats)
    dev.chk(dev.L.s3a_psfwd_decode_queue(dev.h, ps.h, len(feats), ptrs, nfr.ctypes.data_as(PS.P), 0))
    out = []
    for u in range(len(feats)):
        sc, seg = C.c_int32(0), np.zeros((4096, 6), np.int32)
        n = dev.chk(dev.L.s3a_psfwd_queue_hyp(dev.h, u, C.byref(sc), seg.ctypes.data_as(PS.P), 4096))
        out.append((sc.value, [tuple(int(x) for x in seg[i]) for i in range(n)]) if n else (None, []))
    return out


def engine(gpu_lib, desc):
    return PS.Device(gpu_lib, desc, n_lanes=2, max_frames=64, bp_cap=1 << 14, bss_cap=1 << 18)


@pytest.mark.parametrize("ps_overlap", [0, 1])
@pytest.mark.parametrize("n_emit,pl_window", [(3, 0), (3, 2), (5, 0), (5, 2)])
def test_one_psfwd_engine_many_queues(gpu_lib, variants, n_emit, pl_window, ps_overlap):
    variants(ps_overlap=ps_overlap)
    desc, keep = PS.make_desc(5, n_emit=n_emit, pl_window=pl_window)
    assert (desc.n_ci, desc.n_sen) == (10, N_SEN)
    ps, mean = make_scorer(gpu_lib, 11)
    utts = make_utts(12, mean, pl_window)
    calls = [utts[sum(CALLS[:i]):sum(CALLS[:i + 1])] for i in range(len(CALLS))]
    one = engine(gpu_lib, desc)
    for i, feats in enumerate(calls):
        got = decode_queue(one, ps, feats)
        fresh = engine(gpu_lib, desc)
        want = decode_queue(fresh, ps, feats)
        print(f"call {i}: {len(feats)} utterances of {[len(f) for f in feats]} frames, segments {[len(s) for _, s in got]}")
        assert any(seg for _, seg in got), f"call {i}: no hypothesis has segments"
        assert got == want, f"call {i}: the reused engine's hypotheses differ from a fresh engine's"
        del fresh
    # the last call once more as s3a_psfwd_decode (lane z = utterance z, every lane a new decoder)
    feats = calls[-1]
    lock = engine(gpu_lib, desc)
    ptrs, nfr = call_args(feats)
    lock.chk(lock.L.s3a_psfwd_decode(lock.h, ps.h, len(feats), ptrs, nfr.ctypes.data_as(PS.P), 0, 1))
    assert [lock.hyp(z) for z in range(len(feats))] == got


def lextree_snapshot(ls, n_tree):
    return [(ls.active(t, 0).tobytes(), ls.active(t, 1).tobytes(), ls.state(t).tobytes()) for t in range(n_tree)]


def test_lextree_search_and_clones_three_lives(gpu_lib):
    """the recorded tidigits trace (test_gpu_lextree.test_gpu_replays_the_recorded_trace) through a clone, the prototype and a second
    clone; the first clone is freed before the prototype's last use, the second after it"""
    tr = load_lextree_trace()
    seen = []
    for life in range(3):
        proto = make_gpu(gpu_lib, tr)
        first, second = proto.clone(), proto.clone()
        snaps = []
        for ls in (first, proto, second):
            assert lextree_trace.Replayer(tr, ls).run()[0] == 60, life
            snaps.append(lextree_snapshot(ls, tr["n_tree"]))
            if ls is first:
                first.__del__()         # s3a_lexsearch_free now: the static arrays it borrowed stay the prototype's
        second.__del__()
        proto.__del__()
        assert snaps[0] == snaps[1] and snaps[2] == snaps[1], life
        seen.append(snaps[1])
    assert seen[1] == seen[0] and seen[2] == seen[0]


@pytest.mark.parametrize("private_state", [False, True])
def test_scorer_three_lives(gpu_lib, tid, private_state):  # noqa: F811
    """tidigits frames of test_gpu_frame_eval's "default" case; a scorer with the model's Gaussian-selection state leaves it to the model
    when it goes, one with its own state takes that with it"""
    g = golden("tidigits_frame_eval.npz")
    T = 24
    seen = []
    for life in range(3):
        sc = gpu_lib.Scorer(tid, g["cd2cisen"], 102, private_state=private_state)
        r = sc.frame_eval_seq(g["feat"][:T])
        sc.__del__()
        assert np.array_equal(r["ci_best"], g["default_ci_best"][:T]) and np.array_equal(r["best"], g["default_best"][:T]), life
        assert np.array_equal(r["sen_active_out"], g["default_sen_active_out"][:T]), life
        act = r["sen_active_out"].astype(bool)
        assert np.array_equal(r["senscr"][act], g["default_senscr"][:T][act]), life
        assert np.array_equal(r["counts"], g["default_counts"][:T, :2]), life
        if not private_state:           # (frame_eval_seq reads the MODEL's state arrays)
            assert np.array_equal(r["bstidx"], g["default_bstidx"][:T]) and np.array_equal(r["updatetime"], g["default_updatetime"][:T]), life
        seen.append({k: v.tobytes() for k, v in r.items()})
    assert seen[1] == seen[0] and seen[2] == seen[0]


def test_ms_scorer_three_lives(gpu_lib):
    """test_gpu_ms's semi-continuous arrays, top 4"""
    g = golden("ms_mgau.npz")
    seen = []
    for life in range(3):
        ms = gpu_lib.MsMgau.init_arrays(g["semi_mean"], g["semi_var"], g["semi_mixw"], 1, 64, g["semi_featlen"],
                                        gpu_lib.LogMath(1.0003), 4, sen2mgau=np.zeros(200, np.int32))
        scr = np.zeros(200, np.int32)
        got = []
        for t in range(len(g["semi_feat"])):
            sa = g["semi_active"][t]
            best = ms.frame_eval(sa, scr, g["semi_feat"][t], t)
            a = sa.astype(bool)
            assert best == g["semi_top4_best"][t] and np.array_equal(scr[a], g["semi_top4_senscr"][t][a]), (life, t)
            dd, di = ms.last_dist()
            assert np.array_equal(dd, g["semi_top4_dist"][t]) and np.array_equal(di, g["semi_top4_dist_id"][t]), (life, t)
            got.append((best, scr[a].tobytes(), dd.tobytes(), di.tobytes()))
        ms.__del__()
        seen.append(got)
    assert seen[1] == seen[0] and seen[2] == seen[0]
