"""Parity (MI355X): the block entry points of the multi-stream senone scorer -- s3a_ms_mgau_score_frames[_dev],
every senone of many frames in one pass (cmusphinx_amd/csrc/s3a_ms.hip: k_msb_cont for ".s3cont.", k_msb_topn +
k_msb_senone for shared codebooks) -- against the reference's own outputs (tests/golden/ms_mgau.npz) and the CPU
oracle, bit for bit: the rows' active entries and the frame best.  Inactive entries are the caller's."""
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
from cmusphinx_amd import synth
from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu

INT32_MIN = -2 ** 31
SENTINEL = 0x5A5A5A5A
EMPTY_FRAME = 3         # its mask is all zero


@functools.lru_cache(maxsize=None)
def shape_arrays(name):
    """-> dict(mean, var, mixw, M, nd, fl, s2m, feats, masks): the raw arrays of a synthetic shape (built once)"""
    rng = np.random.default_rng(17)
    if name == "cont700":
        m = synth.make_model(n_sen=700, n_ci_sen=50, n_comp=8, veclen=39, n_tmat=8, n_emit=3, seed=11)
        mean, var, mixw = m["mean"], m["var"], m["mixw"]
        M, nd, fl, s2m = 700, 8, [39], None
        feats = synth.make_features(m, 33, seed=9)
    elif name == "semi256":
        fl, nd, M = [12, 24, 3, 12], 256, 1
        D = sum(fl)
        mean = rng.standard_normal(nd * D).astype(np.float32)
        var = np.exp(rng.uniform(np.log(0.05), np.log(2.0), nd * D)).astype(np.float32)
        mixw = (rng.dirichlet(np.ones(nd) * 0.2, (3000, 4)) * 500).astype(np.float32)
        s2m = np.zeros(3000, np.int32)
        feats = (rng.standard_normal((19, D)) * 1.1).astype(np.float32)
    else:
        # "ties_c5": 5 densities (padded to 8 lanes), two streams, 300 senones sharing 40 codebooks; in every third
        # codebook all five densities of stream 0 are identical, so the tie straddles rank topn-1 / topn of a top-3
        # list and only the ids 0, 1, 2 may be listed
        assert name == "ties_c5"
        fl, nd, M = [7, 5], 5, 40
        D = sum(fl)
        mean = np.round(rng.standard_normal(M * nd * D) * 2).astype(np.float32)
        var = np.full(M * nd * D, 0.5, np.float32)
        mean.reshape(40, 60)[::3, 0:35] = np.tile(mean.reshape(40, 60)[::3, 0:7], (1, 5))
        mixw = (rng.dirichlet(np.ones(nd), (300, 2)) * 100).astype(np.float32)
        # a wrong codeword id among the tied densities must change the score: the weights of a senone's densities differ
        assert all(len(np.unique(mixw[s, f])) == nd for s in range(300) for f in range(2))
        assert np.array_equal(mean.reshape(40, 60)[3, 0:7], mean.reshape(40, 60)[3, 28:35])
        s2m = rng.integers(0, M, 300).astype(np.int32)
        feats = np.round(rng.standard_normal((37, D)) * 2).astype(np.float32)
    S = mixw.size // (len(fl) * nd)
    feats = np.ascontiguousarray(feats, np.float32).reshape(-1, sum(fl))
    masks = (rng.random((len(feats), S)) < 0.8).astype(np.uint8)
    masks[EMPTY_FRAME] = 0
    return dict(mean=mean, var=var, mixw=mixw, M=M, nd=nd, fl=fl, s2m=s2m, feats=feats, masks=masks, S=S)


@functools.lru_cache(maxsize=None)
def oracle_rows(name, topn):
    """-> (rows [T][S], best [T]) of the CPU oracle, frame by frame with the shape's masks; never modified"""
    a = shape_arrays(name)
    om = O.OracleMs(a["mean"], a["var"], a["mixw"], a["M"], a["nd"], a["fl"], O.OracleLogMath(1.0003), topn,
                    sen2mgau=a["s2m"])
    rows = np.zeros((len(a["feats"]), a["S"]), np.int32)
    best = np.zeros(len(a["feats"]), np.int64)
    for t in range(len(a["feats"])):
        if t == EMPTY_FRAME:
            continue            # nothing is defined for it but best = INT32_MIN, which the tests state themselves
        best[t], rows[t] = om.frame_eval(a["masks"][t], a["feats"][t])
    rows.setflags(write=False); best.setflags(write=False)
    return rows, best


def gpu_model(gpu_lib, name, topn):
    a = shape_arrays(name)
    return gpu_lib.MsMgau.init_arrays(a["mean"], a["var"], a["mixw"], a["M"], a["nd"], a["fl"], gpu_lib.LogMath(1.0003),
                                      topn, sen2mgau=a["s2m"])


def check_against_oracle(name, topn, rows, best):
    """rows were pre-filled with SENTINEL; best as returned"""
    a = shape_arrays(name)
    orows, obest = oracle_rows(name, topn)
    act = a["masks"].astype(bool)
    assert best[EMPTY_FRAME] == INT32_MIN
    keep = np.arange(len(best)) != EMPTY_FRAME
    assert np.array_equal(best[keep].astype(np.int64), obest[keep]), (name, topn)
    assert np.array_equal(rows[act], orows[act]), (name, topn)
    assert np.all(rows[~act] == np.int32(SENTINEL)), "an inactive entry was written"
    assert np.all(rows[EMPTY_FRAME] == np.int32(SENTINEL))


def sentinel_rows(T, S):
    return np.full((T, S), SENTINEL, np.int32)


# ---- 1, 2: the reference's own dumps -------------------------------------------------------------------------------
@pytest.mark.parametrize("case,topn,masked", [("tid_top8", 8, False), ("tid_top4_masked", 4, True), ("tid_top1", 1, True)])
def test_s3cont_files_match_reference_in_one_call(gpu_lib, case, topn, masked):
    g = golden("ms_mgau.npz")
    d = os.path.join(GOLDEN, "tidigits")
    ms = gpu_lib.MsMgau.init(os.path.join(d, "means"), os.path.join(d, "variances"), os.path.join(d, "mixture_weights"),
                             gpu_lib.LogMath(1.0003), senmgau=".s3cont.", topn=topn)
    T = len(g["feat"])
    assert T == 24
    rows, best = ms.score_frames(g["feat"], g["active"] if masked else None, senscr=sentinel_rows(T, ms.n_sen))
    a = g["active"].astype(bool) if masked else np.ones((T, ms.n_sen), bool)
    assert np.array_equal(best, g[case + "_best"])
    assert np.array_equal(rows[a], g[case + "_senscr"][a])
    assert np.all(rows[~a] == np.int32(SENTINEL))


@pytest.mark.parametrize("case,topn,masked", [("semi_top4", 4, True), ("semi_top64", 64, False)])
def test_semi_arrays_match_reference_in_one_call(gpu_lib, case, topn, masked):
    g = golden("ms_mgau.npz")
    ms = gpu_lib.MsMgau.init_arrays(g["semi_mean"], g["semi_var"], g["semi_mixw"], 1, 64, g["semi_featlen"],
                                    gpu_lib.LogMath(1.0003), topn, sen2mgau=np.zeros(200, np.int32))
    T = len(g["semi_feat"])
    assert T == 12
    rows, best = ms.score_frames(g["semi_feat"], g["semi_active"] if masked else None, senscr=sentinel_rows(T, 200))
    a = g["semi_active"].astype(bool) if masked else np.ones((T, 200), bool)
    assert np.array_equal(best, g[case + "_best"])
    assert np.array_equal(rows[a], g[case + "_senscr"][a])
    assert np.all(rows[~a] == np.int32(SENTINEL))


# ---- 3: synthetic shapes against the oracle ------------------------------------------------------------------------
SHAPES = [("cont700", 1), ("cont700", 4), ("cont700", 8), ("semi256", 4), ("ties_c5", 3)]


@pytest.mark.parametrize("name,topn", SHAPES)
def test_synthetic_shapes_match_oracle(gpu_lib, name, topn):
    a = shape_arrays(name)
    ms = gpu_model(gpu_lib, name, topn)
    rows, best = ms.score_frames(a["feats"], a["masks"], senscr=sentinel_rows(len(a["feats"]), a["S"]))
    check_against_oracle(name, topn, rows, best)


# ---- 4: chunking changes nothing -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,topn", [("ties_c5", 3), ("semi256", 4)])
def test_chunking_changes_nothing(gpu_lib, name, topn):
    a = shape_arrays(name)
    ms = gpu_model(gpu_lib, name, topn)
    got = []
    for chunk in (5, 1, 0):
        ms.set_block_chunk(chunk)
        rows, best = ms.score_frames(a["feats"], a["masks"], senscr=sentinel_rows(len(a["feats"]), a["S"]))
        check_against_oracle(name, topn, rows, best)
        got.append((rows, best))
    for rows, best in got[1:]:
        assert np.array_equal(rows, got[0][0]) and np.array_equal(best, got[0][1])


# ---- 5: agreement with the per-frame entry point -------------------------------------------------------------------
def test_block_call_equals_a_loop_of_frame_eval(gpu_lib):
    a = shape_arrays("cont700")
    ms = gpu_model(gpu_lib, "cont700", 4)
    T, S = len(a["feats"]), a["S"]
    loop_rows, loop_best = sentinel_rows(T, S), np.zeros(T, np.int32)
    for t in range(T):
        loop_best[t] = ms.frame_eval(a["masks"][t], loop_rows[t], a["feats"][t], t)
    rows, best = ms.score_frames(a["feats"], a["masks"], senscr=sentinel_rows(T, S))
    assert np.array_equal(best, loop_best) and np.array_equal(rows, loop_rows)
    # one frame
    r1, b1 = ms.score_frames(a["feats"][7:8], a["masks"][7:8], senscr=sentinel_rows(1, S))
    assert b1[0] == loop_best[7] and np.array_equal(r1[0], loop_rows[7])


# ---- 6: S3A_MS_RAW -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,topn", [("cont700", 4), ("ties_c5", 3)])
def test_raw_rows_minus_best_are_the_normalised_rows(gpu_lib, name, topn):
    a = shape_arrays(name)
    ms = gpu_model(gpu_lib, name, topn)
    T, S = len(a["feats"]), a["S"]
    norm, best = ms.score_frames(a["feats"], a["masks"], senscr=sentinel_rows(T, S))
    raw, rbest = ms.score_frames(a["feats"], a["masks"], raw=True, senscr=sentinel_rows(T, S))
    assert np.array_equal(best, rbest)
    act = a["masks"].astype(bool)
    diff = (raw.view(np.uint32) - best.view(np.uint32)[:, None]).view(np.int32)        # wrapping
    assert np.array_equal(diff[act], norm[act])
    assert np.all(raw[~act] == np.int32(SENTINEL))
    check_against_oracle(name, topn, norm, best)


# ---- 7: everything resident on the device --------------------------------------------------------------------------
@pytest.mark.parametrize("own_stream", [True, False])
@pytest.mark.parametrize("name,topn", [("cont700", 4), ("ties_c5", 3)])
def test_dev_variant_with_strides(gpu_lib, name, topn, own_stream):
    a = shape_arrays(name)
    ms = gpu_model(gpu_lib, name, topn)
    T, S, D = len(a["feats"]), a["S"], ms.veclen
    fs, rs = D + 3, S + 5
    other = None
    stream = None
    if not own_stream:          # a caller's stream: another model's
        lm = gpu_lib.LogMath(1.0003)
        other = gpu_lib.MgauModel.init_arrays(np.ones((2, 2, 4), np.float32), np.ones((2, 2, 4), np.float32),
                                              np.ones((2, 2), np.float32), lm)
        stream = other.stream()
        assert stream
    feat = np.full((T, fs), np.nan, np.float32)
    feat[:, :D] = a["feats"]
    host_rows, host_best = ms.score_frames(a["feats"], a["masks"], senscr=sentinel_rows(T, S))
    fd = gpu_lib.DevBuf(feat.nbytes).upload(feat)
    ad = gpu_lib.DevBuf(a["masks"].nbytes).upload(a["masks"])
    sd = gpu_lib.DevBuf(T * rs * 4).upload(sentinel_rows(T, rs))
    bd = gpu_lib.DevBuf(T * 4).upload(np.zeros(T, np.int32))
    ms.score_frames_dev(fd, T, sd, sen_active_dev=ad, best_dev=bd, feat_stride=fs, row_stride=rs, stream=stream)
    gpu_lib.check(gpu_lib.load().s3a_dev_sync())
    rows, best = sd.download(np.int32, (T, rs)), bd.download(np.int32, (T,))
    assert np.all(rows[:, S:] == np.int32(SENTINEL)), "padding columns were written"
    assert np.array_equal(rows[:, :S], host_rows) and np.array_equal(best, host_best)
    check_against_oracle(name, topn, rows[:, :S].copy(), best)
    # best_dev = NULL
    sd.upload(sentinel_rows(T, rs))
    ms.score_frames_dev(fd, T, sd, sen_active_dev=ad, best_dev=None, feat_stride=fs, row_stride=rs, stream=stream)
    gpu_lib.check(gpu_lib.load().s3a_dev_sync())
    assert np.array_equal(sd.download(np.int32, (T, rs)), rows)
    del other


# ---- 8: argument errors --------------------------------------------------------------------------------------------
def test_argument_errors(gpu_lib):
    a = shape_arrays("ties_c5")
    ms = gpu_model(gpu_lib, "ties_c5", 3)
    S, D = a["S"], ms.veclen
    L = gpu_lib.load()
    fd = gpu_lib.DevBuf(4 * D * 4).upload(a["feats"][:4])
    sd = gpu_lib.DevBuf(4 * S * 4).upload(sentinel_rows(4, S))
    with pytest.raises(gpu_lib.S3AError):
        ms.score_frames_dev(fd, -1, sd)
    with pytest.raises(gpu_lib.S3AError):
        ms.score_frames_dev(fd, 4, sd, row_stride=S - 1)
    with pytest.raises(gpu_lib.S3AError):
        ms.score_frames_dev(fd, 4, sd, feat_stride=D - 1)
    with pytest.raises(gpu_lib.S3AError):
        gpu_lib.check(L.s3a_ms_mgau_score_frames(ms.h, gpu_lib._p(a["feats"]), -1, None,
                                                 gpu_lib._p(sentinel_rows(4, S)), None, 0))
    ms.score_frames_dev(fd, 0, sd)                      # nothing to do: returns cleanly, writes nothing
    gpu_lib.check(L.s3a_dev_sync())
    assert np.all(sd.download(np.int32, (4, S)) == np.int32(SENTINEL))
    rows, best = ms.score_frames(np.zeros((0, D), np.float32))
    assert rows.shape == (0, S) and best.shape == (0,)
