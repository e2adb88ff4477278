"""Rows ahead (kf_decode_queue / kf_launch_overlapped, s3a_variants_t.kf_overlap_lead / _round / _whole / _hold): of the first n1 takes'
utterances only a LEAD is scored before the search begins; the companion scores their later frames beside it in ROUNDS (R groups of 8
frames of each utterance per launch), a device word *f_ready says how far all of them are scored, and a lane that reaches a frame at or
beyond it LEAVES at that frame boundary -- the launch behind the scoring continues the utterance there.  Nothing of this may change a bit:

  rounds at their smallest (R = 1, a lead of 8 frames), twice on one engine; with kf_overlap_hold every first lane runs to its lead and
  leaves inside its utterance (the count is known from the lengths); the edges of the gate (utterances shorter than, as long as and one
  frame longer than the lead); the relay's hand-overs behind lanes that were resumed inside an utterance; RM1; the A/B switch.

Hold only changes the ORDER of the work enqueued on the two streams (every fill of the second stream and the second launch wait for the
first launch's end): what otherwise is a race between two streams is then the same on every run.

Expected output: the reference's committed -hyp / -hypseg lines, and the same engine with kf_no_overlap = 1, record for record."""
import pytest

import test_gpu_queue as TQ
from cmusphinx_amd import bundle
from test_gpu_kf_overlap import KF, records, rm1, same_records  # noqa: F401  (rm1: fixture)
from test_gpu_uttdec import tidigits_bundle  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tidigits_plain(gpu_lib, tidigits_bundle):
    """the 31 utterances, the reference's lines, and the records of an 8-lane engine that scores everything first -- made once"""
    from cmusphinx_amd import lib
    utts, feats = TQ.tidigits_feats(gpu_lib)
    rm, rs = TQ.ref_lines()
    lib.set_variants(kf_no_overlap=1)
    try:
        plain = bundle.Decoder(tidigits_bundle, 8, opts=KF)
        plain.decode_queue(feats)
        assert plain.ud.last_overlap()["overlapped"] == 0
        want = records(plain, len(feats))
    finally:
        lib.set_variants()
    return utts, feats, rm, rs, want


def check_tidigits(dec, utts, feats, rm, rs, want):
    m, s = TQ.queue_lines(dec, utts)
    assert m == rm and s == rs
    assert same_records(records(dec, len(feats)), want)
    assert dec.ud.last_overlap()["overlapped"] == 1


def test_rounds_at_their_smallest(tidigits_plain, tidigits_bundle, variants):
    """one group of each first utterance per launch, a lead of one group; twice on one engine (the words and the lanes' flags are reset)"""
    utts, feats, rm, rs, want = tidigits_plain
    variants(kf_overlap_n1=4, kf_overlap_round=1, kf_overlap_lead=8)
    dec = bundle.Decoder(tidigits_bundle, 8, opts=KF)
    longest4 = sorted((len(f) for f in feats), reverse=True)[:4]
    for _ in range(2):
        dec.decode_queue(feats)
        check_tidigits(dec, utts, feats, rm, rs, want)
        o2 = dec.ud.last_overlap2()
        assert o2["lead"] == 8 and 0 <= o2["left_inside"] <= 4, o2
        # (a launch per round of the longest first utterance behind the lead's, and at least one for the other 27 utterances)
        assert dec.ud.last_parts()["n_score"] >= 1 + ((longest4[0] + 7) // 8 - 1) + 1, dec.ud.last_parts()
        print(f"{o2['left_inside']} lanes left inside an utterance, {dec.ud.last_overlap()['resumed']} were resumed")


@pytest.mark.parametrize("lead", [8, 16])
def test_every_first_lane_leaves_inside_its_utterance(tidigits_plain, tidigits_bundle, variants, lead):
    utts, feats, rm, rs, want = tidigits_plain
    variants(kf_overlap_n1=4, kf_overlap_round=1, kf_overlap_lead=lead, kf_overlap_hold=1)
    dec = bundle.Decoder(tidigits_bundle, 8, opts=KF)
    first4 = sorted((len(f) for f in feats), reverse=True)[:4]
    expect = sum(1 for n in first4 if n > lead)
    assert expect == 4
    dec.decode_queue(feats)
    check_tidigits(dec, utts, feats, rm, rs, want)
    o2, ov = dec.ud.last_overlap2(), dec.ud.last_overlap()
    assert o2 == dict(left_inside=expect, lead=lead), o2
    assert ov["resumed"] == 4, ov


def test_edges_of_the_gate(gpu_lib, tidigits_bundle, variants):
    """the queue in ITS order; its first takes: copies cut to 3 frames, to exactly the lead (8) and to 9 frames, then the first whole
    utterance.  With hold nothing beyond the lead is scored while the first launch runs: the 3-frame and the 8-frame copy never ask for an
    unscored frame and end as the plain engine ends them (their lanes then leave BETWEEN utterances: no scored take is left); the 9-frame
    copy has one frame at or beyond the lead, frame 8, and leaves there, as the whole utterance does: two lanes inside."""
    utts, feats = TQ.tidigits_feats(gpu_lib)
    assert len(feats[3]) > 9
    queue = [feats[0][:3].copy(), feats[1][:8].copy(), feats[2][:9].copy()] + feats
    variants(kf_queue_in_order=1, kf_no_overlap=1)
    plain = bundle.Decoder(tidigits_bundle, 8, opts=KF)
    plain.decode_queue(queue)
    want = records(plain, len(queue))
    variants(kf_queue_in_order=1, kf_overlap_n1=4, kf_overlap_round=1, kf_overlap_lead=8, kf_overlap_hold=1)
    dec = bundle.Decoder(tidigits_bundle, 8, opts=KF)
    dec.decode_queue(queue)
    assert dec.ud.last_overlap()["overlapped"] == 1
    assert same_records(records(dec, len(queue)), want)
    for q, f in enumerate(queue):
        h, _ = dec.queue_hyp(q, f"u{q}", q)
        assert h.n_frames == len(f), q
    rm, rs = TQ.ref_lines()
    got = [dec.format_var(*dec.queue_hyp(3 + k, utts[k][1], k)) for k in range(len(feats))]
    assert [g[0] for g in got] == rm and [g[1] for g in got] == rs
    assert dec.ud.last_overlap2() == dict(left_inside=2, lead=8)
    assert dec.ud.last_overlap()["resumed"] == 4            # (the two that left inside, the two that found no scored take)


def test_with_the_relay_behind_it(gpu_lib, tidigits_bundle, variants):
    """16 lanes, the first 8 run to their lead and leave; the second launch resumes them inside their utterances and the relay hands the
    last lanes over later: lane_f / lane_uq serve both"""
    utts, feats = TQ.tidigits_feats(gpu_lib)
    rm, rs = TQ.ref_lines()
    variants(kf_overlap_n1=8, kf_relay_at=8, kf_overlap_hold=1, kf_overlap_round=1)
    dec = bundle.Decoder(tidigits_bundle, 16, opts=KF)
    dec.decode_queue(feats)
    m, s = TQ.queue_lines(dec, utts)
    assert m == rm and s == rs
    assert dec.ud.last_overlap()["overlapped"] == 1 and dec.ud.last_relay() == 2
    o2 = dec.ud.last_overlap2()
    first8 = sorted((len(f) for f in feats), reverse=True)[:8]
    assert o2["left_inside"] == sum(1 for n in first8 if n > o2["lead"]) and o2["lead"] % 8 == 0 and o2["lead"] > 0, o2
    variants(kf_no_overlap=1, kf_no_relay=1)
    plain = bundle.Decoder(tidigits_bundle, 16, opts=KF)
    plain.decode_queue(feats)
    assert same_records(records(dec, len(feats)), records(plain, len(feats)))


def test_rm1_once(gpu_lib, rm1, variants):
    b, utts, feats, rm, rs = rm1
    variants(kf_no_overlap=1)
    plain = bundle.Decoder(b, 8, opts=KF)
    plain.decode_queue(feats)
    want = records(plain, len(feats))
    for hold in (0, 1):
        variants(kf_overlap_n1=4, kf_overlap_round=1, kf_overlap_hold=hold)
        dec = bundle.Decoder(b, 8, opts=KF)
        dec.decode_queue(feats)
        m, s = TQ.queue_lines(dec, utts)
        assert m == rm and s == rs, hold
        assert dec.ud.last_overlap()["overlapped"] == 1
        assert same_records(records(dec, len(feats)), want), hold
        o2 = dec.ud.last_overlap2()
        if hold:
            first4 = sorted((len(f) for f in feats), reverse=True)[:4]
            assert o2["left_inside"] == sum(1 for n in first4 if n > o2["lead"]), o2


def test_the_ab_switch(tidigits_plain, tidigits_bundle, variants):
    """kf_overlap_whole: the first utterances scored whole up front, no lane can leave inside one -- with and without hold"""
    utts, feats, rm, rs, want = tidigits_plain
    for hold in (0, 1):
        variants(kf_overlap_n1=4, kf_overlap_whole=1, kf_overlap_hold=hold)
        dec = bundle.Decoder(tidigits_bundle, 8, opts=KF)
        dec.decode_queue(feats)
        check_tidigits(dec, utts, feats, rm, rs, want)
        assert dec.ud.last_overlap2() == dict(left_inside=0, lead=0)
