"""Scoring beside the search (kf_decode_queue, s3a_variants_t.kf_overlap / kf_overlap_n1 / kf_no_overlap / uw_companion): a queue's
first n1 lanes start on the n1 longest utterances while a COMPANION shape of the scoring kernel (256 threads, the LDS a CU has left
beside a ku_frames workgroup) scores the rest on a second stream; the other lanes start behind it, and a lane of the first launch
whose next take is not scored yet LEAVES and is taken up again by a launch behind the scoring.  Nothing of this may change a bit:

  the companion shape alone (every up-front pass through it, no concurrency), the plan forced onto 8-lane engines (n1 = 4), lanes
  that do leave (the first takes are utterances of 1 and 2 frames), the calls the plan must leave alone (no more utterances than
  lanes, a queue in parts, the second pass), and the plan with the relay's hand-overs behind it.

Expected output: the reference's committed -hyp / -hypseg lines (tidigits_decode; rm1_decode: RM1's files are unpacked by
tests/local_data.py), and the same engine with the switches off, record for record."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_dropin as TD
import test_gpu_queue as TQ
from cmusphinx_amd import bundle, lib, s3io
from conftest import GOLDEN
from test_gpu_uttdec import TST, tidigits_bundle  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

KF = {"persist": 1}             # ku_frames whatever the lane count


@pytest.fixture(scope="module")
def rm1(tmp_path_factory):
    """RM1's 20 utterances: the bundle (exported by the drop-in program, one utterance decoded along the way), the features, and the
    unmodified reference's lines (tests/golden/rm1_decode: sphinx3_decode with test_gpu_dropin.rm_args(), which
    test_gpu_dropin.py::test_rm1_identical_to_live_reference reproduces live) -- made once for the module"""
    d = tmp_path_factory.mktemp("rm1")
    one = TD.rm_args()
    one[one.index("-ctlcount") + 1] = "1"
    out = str(d / "rm1.bundle")
    p = subprocess.run([TST] + one, env=dict(os.environ, S3A_UTT="1", S3A_EXPORT=out), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                       timeout=900)
    assert p.returncode == 0 and os.path.getsize(out) > 1000
    ids = [l.split()[0] for l in open(f"{TD.RM}/rm.ctl") if l.split()][:20]
    feats = [lib.feat_1s_c_d_dd(s3io.read_mfc(f"{TD.RM}/feat/{u}.mfc").reshape(-1, 13), cmn="current") for u in ids]
    utts = [(u, os.path.basename(u)) for u in ids]
    g = os.path.join(GOLDEN, "rm1_decode")
    rm = open(f"{g}/ref_mode4_trigram.match").read().splitlines(keepends=True)
    rs = open(f"{g}/ref_mode4_trigram.matchseg").read().splitlines(keepends=True)
    assert len(rm) == 20 and len(rs) == 20
    return out, utts, feats, rm, rs


def records(dec, n):
    return [(bytes(h), np.array(w)) for h, w in (dec.queue_hyp(q, f"u{q}", q) for q in range(n))]


def same_records(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def test_companion_kernel_alone_tidigits(gpu_lib, tidigits_bundle, variants):
    """every up-front scoring pass through the companion shape, nothing concurrent: the reference's lines, the plain engine's records"""
    utts, feats = TQ.tidigits_feats(gpu_lib)
    rm, rs = TQ.ref_lines()
    plain = bundle.Decoder(tidigits_bundle, 8, opts=KF)
    plain.decode_queue(feats)
    want = records(plain, len(feats))
    variants(uw_companion=1, kf_no_overlap=1)
    dec = bundle.Decoder(tidigits_bundle, 8, opts=KF)
    dec.decode_queue(feats)
    m, s = TQ.queue_lines(dec, utts)
    assert m == rm and s == rs
    assert same_records(records(dec, len(feats)), want)
    assert dec.ud.last_overlap()["overlapped"] == 0 and dec.ud.last_parts()["n_score"] >= 1


def test_companion_kernel_alone_rm1(gpu_lib, rm1, variants):
    b, utts, feats, rm, rs = rm1
    plain = bundle.Decoder(b, 8, opts=KF)
    plain.decode_queue(feats)
    want = records(plain, len(feats))
    m, s = TQ.queue_lines(plain, utts)
    assert m == rm and s == rs
    variants(uw_companion=1, kf_no_overlap=1)
    dec = bundle.Decoder(b, 8, opts=KF)
    dec.decode_queue(feats)
    m, s = TQ.queue_lines(dec, utts)
    assert m == rm and s == rs
    assert same_records(records(dec, len(feats)), want)


def test_overlap_forced_tidigits(gpu_lib, tidigits_bundle, variants):
    """31 utterances, 8 lanes, the first 4 lanes beside the companion's scoring of the other 27 utterances; twice on one engine"""
    utts, feats = TQ.tidigits_feats(gpu_lib)
    rm, rs = TQ.ref_lines()
    variants(kf_no_overlap=1)
    plain = bundle.Decoder(tidigits_bundle, 8, opts=KF)
    plain.decode_queue(feats)
    want = records(plain, len(feats))
    assert plain.ud.last_overlap()["overlapped"] == 0
    variants(kf_overlap_n1=4)
    dec = bundle.Decoder(tidigits_bundle, 8, opts=KF)
    for _ in range(2):
        dec.decode_queue(feats)
        m, s = TQ.queue_lines(dec, utts)
        assert m == rm and s == rs
        assert same_records(records(dec, len(feats)), want)
        assert dec.ud.last_overlap()["overlapped"] == 1
        parts = dec.ud.last_parts()
        assert parts["score_ms"] > 0 and parts["frames_ms"] > 0 and parts["n_score"] >= 2 and parts["n_frames"] == 1 and parts["cluster"] == 1, parts


def test_overlap_forced_rm1(gpu_lib, rm1, variants):
    b, utts, feats, rm, rs = rm1
    variants(kf_overlap_n1=4)
    dec = bundle.Decoder(b, 8, opts=KF)
    dec.decode_queue(feats)
    m, s = TQ.queue_lines(dec, utts)
    assert m == rm and s == rs
    assert dec.ud.last_overlap()["overlapped"] == 1
    variants(kf_no_overlap=1)
    plain = bundle.Decoder(b, 8, opts=KF)
    plain.decode_queue(feats)
    assert same_records(records(dec, len(feats)), records(plain, len(feats)))


def test_a_lane_that_leaves_is_taken_up_again(gpu_lib, tidigits_bundle, variants):
    """the queue in ITS order, its first four takes utterances of 1 and 2 frames: the first launch's lanes are through with them long
    before the other 27 utterances are scored, find their next take not scored, leave, and the launch behind the scoring takes them up
    again.  Every utterance's record once and as the plain engine writes it (the four short ones: the failure status the reference has
    for them too).  Whether a lane did leave is a race between two streams: reported, and said plainly when it went the other way."""
    utts, feats = TQ.tidigits_feats(gpu_lib)
    queue = [feats[0][:1].copy(), feats[1][:2].copy(), feats[2][:1].copy(), feats[3][:2].copy()] + feats
    variants(kf_queue_in_order=1, kf_no_overlap=1)
    plain = bundle.Decoder(tidigits_bundle, 8, opts=KF)
    plain.decode_queue(queue)
    want = records(plain, len(queue))
    variants(kf_queue_in_order=1, kf_overlap_n1=4)
    dec = bundle.Decoder(tidigits_bundle, 8, opts=KF)
    dec.decode_queue(queue)
    ov = dec.ud.last_overlap()
    assert ov["overlapped"] == 1
    got = records(dec, len(queue))
    assert same_records(got, want)
    for q, f in enumerate(queue):
        h, _ = dec.queue_hyp(q, f"u{q}", q)
        assert h.n_frames == len(f), q                      # every utterance was decoded (its header was written) ...
        assert (h.status != 0) == (q < 4), q                # ... the short ones as the reference ends them
    rm, rs = TQ.ref_lines()
    m, s = {}, {}
    for k in range(len(feats)):
        m[k], s[k] = dec.format_var(*dec.queue_hyp(4 + k, utts[k][1], k))
    assert [m[k] for k in range(len(feats))] == rm and [s[k] for k in range(len(feats))] == rs
    if ov["resumed"] > 0:
        print(f"{ov['resumed']} lanes left for want of scores and were resumed")
    else:
        print("the race went the other way on this run: the rest was scored before any first lane asked for its next utterance")
    assert 0 <= ov["resumed"] <= 4


def test_calls_the_plan_leaves_alone(gpu_lib, tidigits_bundle, variants, monkeypatch):
    """no more utterances than lanes; a queue whose scores go through the buffer in parts; a queue with the second pass"""
    utts, feats = TQ.tidigits_feats(gpu_lib)
    rm, rs = TQ.ref_lines()
    variants(kf_overlap_n1=4)
    dec = bundle.Decoder(tidigits_bundle, 8, opts=KF)
    dec.decode_queue(feats[:8])
    m, s = TQ.queue_lines(dec, utts[:8])
    assert m == rm[:8] and s == rs[:8] and dec.ud.last_overlap() == dict(overlapped=0, resumed=0)
    longest, total = max(len(f) for f in feats), sum(len(f) for f in feats)
    parts = bundle.Decoder(tidigits_bundle, 8, opts=dict(KF, score_rows_max=max(longest, total // 3)))
    parts.decode_queue(feats)
    m, s = TQ.queue_lines(parts, utts)
    assert m == rm and s == rs and parts.ud.last_overlap()["overlapped"] == 0 and parts.ud.last_parts()["n_frames"] >= 2
    want = bundle.Decoder(tidigits_bundle, 4, bestpath=True, opts=KF)
    variants(kf_no_overlap=1)
    want.decode_queue(feats[:12])
    w = [want.queue_bestpath_hyp(u, utts[u][1], u) for u in range(12)]
    variants(kf_overlap_n1=2)
    bp = bundle.Decoder(tidigits_bundle, 4, bestpath=True, opts=KF)
    bp.decode_queue(feats[:12])
    assert bp.ud.last_overlap()["overlapped"] == 0
    for u in range(12):
        h, ws = bp.queue_bestpath_hyp(u, utts[u][1], u)
        assert h.status == 0 and bytes(h) == bytes(w[u][0]) and np.array_equal(ws, w[u][1]), u


def test_overlap_with_the_relay_behind_it(gpu_lib, tidigits_bundle, variants):
    """16 lanes, the first 8 beside the scoring, and the relay's hand-overs at 8 and 4 lanes behind the three launches"""
    utts, feats = TQ.tidigits_feats(gpu_lib)
    rm, rs = TQ.ref_lines()
    variants(kf_overlap_n1=8, kf_relay_at=8)
    dec = bundle.Decoder(tidigits_bundle, 16, opts=KF)
    dec.decode_queue(feats)
    m, s = TQ.queue_lines(dec, utts)
    assert m == rm and s == rs
    assert dec.ud.last_overlap()["overlapped"] == 1 and dec.ud.last_relay() == 2
    variants(kf_no_overlap=1, kf_no_relay=1)
    plain = bundle.Decoder(tidigits_bundle, 16, opts=KF)
    plain.decode_queue(feats)
    assert same_records(records(dec, len(feats)), records(plain, len(feats)))
