/* The host's SCHEDULE of a queue call (s3a_utt.hip: s3a_uttdec_decode_queue), as data: arithmetic on the utterances' lengths alone -- no
 * device, no engine -- so that it can be checked without a GPU (s3a_queue_events, tests/test_queue_events.py).  Which lane decodes which
 * utterance from which engine frame on, under which scan epoch; what the lanes are left with; and the EVENTS the host enqueues between
 * frames: the lanes whose utterances end (their hypotheses, the second pass, lextree_utt_end) and the lanes that begin one
 * (srch_TST_begin + the utterance's staged context), as offsets into one flat array of lane / utterance lists that goes to the device.
 *
 * The two forms:
 *   q_sched_refill  the launch routes (graph blocks, window blocks, launches per frame).  The first n_lanes utterances start at engine
 *                   frame 0; from then on, at every multiple of `boundary` frames, every lane whose utterance has ended takes the queue's
 *                   next one (lanes in index order).  An utterance that starts at f0 with n frames ends at the first boundary at or behind
 *                   f0 + n.  One event per boundary at which something ends or begins, in increasing frame order; in an event the ends come
 *                   before the begins (a lane may end one utterance and begin the next in the same event), each in queue order; max_nfr:
 *                   the longest of the BEGINNING utterances (what -pheurtype's tables are made for).  The last event only ends lanes: its
 *                   frame is f_end.  Scan epochs: k_dec_scan's flags are never reset, so a lane's stamps keep growing -- a lane starts at
 *                   max(epoch0[z], 1), an utterance gets its lane's epoch and the lane moves on by the utterance's frames + 1.
 *   q_sched_groups  the second-pass / -pheurtype queue as groups of static ku_frames launches: per part of the KfPlan (KFP_LANES) lane z
 *                   decodes the part's z-th take from its first frame to its last.  One event per part, its lanes ending what they begin:
 *                   o_end == o_beg.  Every epoch is 1 and every f0 is 0 (ku_frames stamps nothing and knows no engine frame); a lane
 *                   keeps the utterance of the last part that has it.
 * A QSched as constructed is the plain ku_frames queue's, where the lanes take the utterances themselves: no lane is anyone's, no events.
 * lists: per event [ending lanes][their utterances] at o_end, [beginning lanes][their utterances] at o_beg. */
#ifndef S3A_QSCHED_H
#define S3A_QSCHED_H
#include <stdint.h>
#include <limits.h>
#include <vector>
#include <algorithm>
#include "s3a_kfplan.h"

struct QEvent { int32_t f, o_end, o_beg, n_end, n_beg, max_nfr; };
struct QSched {
    std::vector<int32_t> lane, f0, epoch;                       /* [n_utt] (lane -1: whichever takes it) */
    std::vector<int32_t> last_utt, epoch_after, nfr_after;      /* [lanes] the lane's last utterance (-1: none) | where its epoch has come
                                                                 * to at least | what HostLane::nfr ends as */
    std::vector<QEvent> events;
    std::vector<int32_t> lists;
    int32_t f_end = 0;                                          /* engine frames of the call (q_sched_refill: -1 = bad arguments) */
    QSched(int32_t n_utt, int32_t n_lanes)
        : lane((size_t)n_utt, -1), f0((size_t)n_utt, 0), epoch((size_t)n_utt, 1), last_utt((size_t)n_lanes, -1),
          epoch_after((size_t)n_lanes, 1), nfr_after((size_t)n_lanes, 0) {}
};

static inline QSched
q_sched_refill(int32_t n_lanes, int32_t boundary, int32_t n_utt, const int32_t *n_frames, const int32_t *epoch0)
{
    const int32_t n = std::min(n_lanes, n_utt);
    QSched Q(std::max(n_utt, 0), std::max(n, 0));
    Q.f_end = -1;
    if (n_lanes <= 0 || boundary <= 0 || n_utt <= 0 || !n_frames) return Q;
    for (int32_t u = 0; u < n_utt; u++) if (n_frames[u] <= 0) return Q;
    /* who runs where from when */
    std::vector<int32_t> busy_until((size_t)n, 0);
    std::vector<char> busy((size_t)n, 0);
    int32_t next = 0;
    for (long long F = 0;; F += boundary) {
        if (F > INT_MAX - boundary) return Q;
        bool any = false;
        for (int32_t z = 0; z < n; z++) {
            if (busy[z] && busy_until[z] <= F) busy[z] = 0;
            if (!busy[z] && next < n_utt) {
                Q.lane[next] = z; Q.f0[next] = (int32_t)F;
                busy_until[z] = (int32_t)F + n_frames[next]; busy[z] = 1;
                next++;
            }
            any = any || busy[z];
        }
        if (!any) { Q.f_end = (int32_t)F; break; }
    }
    /* the lanes' epochs, and who ends and who begins at which boundary: a mark per end and per begin, sorted by frame, ends first (stable:
     * queue order = the order of a lane's utterances) */
    struct Mark { int32_t f, begins, u; };
    std::vector<Mark> marks;
    marks.reserve((size_t)2 * n_utt);
    for (int32_t z = 0; z < n; z++) Q.epoch_after[z] = std::max(epoch0 ? epoch0[z] : 0, 1);
    for (int32_t u = 0; u < n_utt; u++) {
        const int32_t z = Q.lane[u];
        Q.epoch[u] = Q.epoch_after[z];
        Q.epoch_after[z] += n_frames[u] + 1;
        Q.nfr_after[z] = n_frames[u];
        Q.last_utt[z] = u;
        marks.push_back({ Q.f0[u], 1, u });
        marks.push_back({ (int32_t)(((int64_t)Q.f0[u] + n_frames[u] + boundary - 1) / boundary * boundary), 0, u });
    }
    std::stable_sort(marks.begin(), marks.end(), [](const Mark &a, const Mark &b) { return a.f != b.f ? a.f < b.f : a.begins < b.begins; });
    for (size_t i = 0; i < marks.size(); ) {
        size_t j = i, k;
        while (j < marks.size() && marks[j].f == marks[i].f && !marks[j].begins) j++;
        for (k = j; k < marks.size() && marks[k].f == marks[i].f; ) k++;
        QEvent e = { marks[i].f, (int32_t)Q.lists.size(), 0, (int32_t)(j - i), (int32_t)(k - j), 0 };
        for (size_t m = i; m < j; m++) Q.lists.push_back(Q.lane[marks[m].u]);
        for (size_t m = i; m < j; m++) Q.lists.push_back(marks[m].u);
        e.o_beg = (int32_t)Q.lists.size();
        for (size_t m = j; m < k; m++) { Q.lists.push_back(Q.lane[marks[m].u]); e.max_nfr = std::max(e.max_nfr, n_frames[marks[m].u]); }
        for (size_t m = j; m < k; m++) Q.lists.push_back(marks[m].u);
        Q.events.push_back(e);
        i = k;
    }
    return Q;
}

/* K: kf_plan(n_utt, n_frames, KFP_LANES, n_lanes, ...) */
static inline QSched
q_sched_groups(const KfPlan &K, const int32_t *n_frames, int32_t n_lanes)
{
    const int32_t n_utt = (int32_t)K.order.size();
    QSched Q(n_utt, std::min(n_lanes, n_utt));
    for (size_t p = 0; p + 1 < K.cut.size(); p++) {
        const int32_t k0 = K.cut[p], m = K.cut[p + 1] - k0, o = (int32_t)Q.lists.size();
        QEvent e = { 0, o, o, m, m, 0 };
        for (int32_t z = 0; z < m; z++) Q.lists.push_back(z);
        for (int32_t z = 0; z < m; z++) {
            const int32_t u = K.order[k0 + z];
            Q.lists.push_back(u);
            Q.lane[u] = z; Q.last_utt[z] = u;
            e.max_nfr = std::max(e.max_nfr, n_frames[u]);
        }
        Q.events.push_back(e);
    }
    return Q;
}
#endif
