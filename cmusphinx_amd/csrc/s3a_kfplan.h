/* The host's PLAN of a ku_frames call (s3a_utt.hip: kf_decode_queue, kf_decode_static, the second-pass / -pheurtype queue), as data:
 * arithmetic on the utterances' lengths alone -- no device, no engine -- so that it can be checked without a GPU (s3a_kf_queue_plan,
 * tests/test_kf_plan.py).  A call's utterances go through in PARTS; inside a part the lanes TAKE the utterances in `order`; every frame of
 * a part's utterances has a ROW of senone scores (rows restart at 0 in every part), scored in GROUPS of 8 consecutive frames of one
 * utterance; the groups' table is uploaded once, in the order the scoring launches walk it.
 *
 * The three callers' rules:
 *   KFP_BUDGET  the plain queue: a part is consecutive utterances whose rows fit `budget`; inside a part the longest utterance is taken
 *               first (stable: equal lengths in queue order -- the launch ends with its slowest lane, and an utterance taken when the
 *               counter is nearly through should be a short one), or, in_order, the queue's order is the takes'.  Rows and groups run
 *               in QUEUE order inside a part (the lanes look their rows up by utterance, any order serves) -- unless the part is scored
 *               BESIDE the search (n1 > 0), which needs what is taken first scored first: then in take order.
 *   KFP_LANES   the second-pass queue: the WHOLE queue longest first, then parts of `budget` = n_lanes takes (lane z of a part decodes
 *               its z-th take); rows and groups in take order.
 *   KFP_ONE     kf_decode_static: one part, lane z decodes utterance z (KFP_LANES with identity order and n_utt lanes).
 * row0[]: an utterance's first row.  KFP_BUDGET: by UTTERANCE (row0[u]; ku_frames' KF_QUEUE looks up what it took); KFP_LANES / KFP_ONE:
 * by TAKE (row0[k] is order[k]'s; KF_STATIC's lane z of the part that begins at take k0 reads row0[k0 + z]).
 *
 * Scoring beside the search (n1 > 0; one part of KFP_BUDGET, fewer first takes than utterances, else ignored): the first n1 takes'
 * groups come first, ROUND by round -- the first lead_groups groups of each of them (the LEAD, scored before the search begins), then the
 * next round_groups of each, and so on, an utterance that has ended skipped; `whole`: no rounds, each of them whole --, then the other
 * takes' groups in take order; one run of rows over both.  The second stream's SCRIPT is what follows the lead: scoring launches of at
 * most KFP_PIECE groups, with *f_ready (frames [0, min(v, length)) of EVERY first take are scored; INT32_MAX behind the last round) and
 * *q_ready (the takes [0, v) are scored whole) moved on behind them as soon as the table's order allows. */
#ifndef S3A_KFPLAN_H
#define S3A_KFPLAN_H
#include <stdint.h>
#include <vector>
#include <algorithm>

#define KFP_FB 8            /* frames of a group (the scoring kernel's UW_FB) */
#define KFP_PIECE 1024      /* groups of a scoring launch at most */
enum { KFP_BUDGET = 0, KFP_LANES = 1, KFP_ONE = 2 };
enum { KFP_SCORE = 0, KFP_F_READY = 1, KFP_Q_READY = 2 };

struct KfGroup { int32_t utt, first, frames; int64_t row; };    /* frames [first, first + frames) of utt into rows [row, row + frames) */
struct KfStep { int32_t op; int64_t a, b; };                    /* KFP_SCORE: the table's groups [a, b) | KFP_F_READY, KFP_Q_READY: = a */
struct KfPlan {
    std::vector<int32_t> order, cut;        /* [n_utt] the takes | [parts + 1] the parts' takes [cut[p], cut[p + 1]) */
    std::vector<int64_t> row0;              /* [n_utt] (indexing: above) */
    std::vector<KfGroup> groups;            /* upload order */
    std::vector<size_t> g_at;               /* [parts + 1] the parts' groups [g_at[p], g_at[p + 1]) */
    size_t max_rows = 0;                    /* the largest part's rows */
    int32_t n1 = 0;                         /* first takes scored beside the search (0: none, nothing below) */
    size_t g_first = 0, g_lead = 0;         /* their groups [0, g_first) | scored before the search begins: [0, g_lead) */
    int32_t lead = 0, f_ready0 = 0;         /* frames of the lead (whole: 0) | *f_ready when the search begins */
    std::vector<KfStep> script;
};

static inline KfPlan
kf_plan(int32_t n_utt, const int32_t *len, int32_t rule, size_t budget, bool in_order, int32_t n1, int32_t lead_groups, int32_t round_groups, bool whole)
{
    KfPlan P;
    if (rule == KFP_ONE) { rule = KFP_LANES; budget = (size_t)n_utt; in_order = true; }
    const auto longer = [&](int32_t a, int32_t b) { return len[a] > len[b]; };
    const auto n_groups = [&](int32_t u) { return (int64_t)((len[u] + KFP_FB - 1) / KFP_FB); };
    P.order.resize((size_t)n_utt);
    for (int32_t u = 0; u < n_utt; u++) P.order[u] = u;
    P.cut.assign(1, 0);
    if (rule == KFP_LANES) {
        if (!in_order) std::stable_sort(P.order.begin(), P.order.end(), longer);
        for (size_t k = std::max(budget, (size_t)1); k < (size_t)n_utt; k += std::max(budget, (size_t)1)) P.cut.push_back((int32_t)k);
    }
    else {
        size_t rows = 0;
        for (int32_t u = 0; u < n_utt; u++) {
            if (rows > 0 && rows + (size_t)len[u] > budget) { P.cut.push_back(u); rows = 0; }
            rows += (size_t)len[u];
        }
    }
    P.cut.push_back(n_utt);
    const size_t parts = P.cut.size() - 1;
    if (rule == KFP_BUDGET && !in_order)
        for (size_t p = 0; p < parts; p++) std::stable_sort(P.order.begin() + P.cut[p], P.order.begin() + P.cut[p + 1], longer);
    P.n1 = n1 = rule == KFP_BUDGET && parts == 1 && n1 > 0 && n1 < n_utt ? n1 : 0;

    /* rows: the k-th utterance of a part's run of rows is its k-th take, or (above) the queue's k-th */
    const bool by_take = rule == KFP_LANES, take_rows = by_take || n1 > 0;
    const auto at = [&](int32_t k) { return take_rows ? P.order[k] : k; };
    P.row0.assign((size_t)n_utt, 0);
    int64_t total_groups = 0;
    for (size_t p = 0; p < parts; p++) {
        int64_t row = 0;
        for (int32_t k = P.cut[p]; k < P.cut[p + 1]; k++) {
            P.row0[by_take ? k : at(k)] = row;
            row += len[at(k)];
            total_groups += n_groups(at(k));
        }
        P.max_rows = std::max(P.max_rows, (size_t)row);
    }
    /* the groups [a, b) of the k-th utterance of the rows' order */
    P.groups.reserve((size_t)total_groups);
    const auto describe = [&](int32_t k, int64_t a, int64_t b) {
        const int32_t u = at(k);
        const int64_t r0 = P.row0[by_take ? k : u];
        for (int64_t f = a * KFP_FB; f < std::min(b * KFP_FB, (int64_t)len[u]); f += KFP_FB)
            P.groups.push_back({ u, (int32_t)f, (int32_t)std::min((int64_t)KFP_FB, len[u] - f), r0 + f });
    };
    P.g_at.assign(1, 0);
    if (n1 == 0) {
        for (size_t p = 0; p < parts; p++) {
            for (int32_t k = P.cut[p]; k < P.cut[p + 1]; k++) describe(k, 0, n_groups(at(k)));
            P.g_at.push_back(P.groups.size());
        }
        return P;
    }
    /* the first n1 takes round by round: rd_g[r] = where round r begins in the table, rd_f[r] = the frames scored once it is */
    std::vector<size_t> rd_g(1, 0);
    std::vector<int32_t> rd_f;
    int64_t max_g = 0;
    for (int32_t k = 0; k < n1; k++) max_g = std::max(max_g, n_groups(P.order[k]));
    for (int64_t a = 0; a < max_g && !whole; ) {
        const int64_t b = std::min(max_g, a + std::max(1, a == 0 ? lead_groups : round_groups));
        for (int32_t k = 0; k < n1; k++) describe(k, a, b);
        rd_g.push_back(P.groups.size()); rd_f.push_back((int32_t)(b * KFP_FB));
        a = b;
    }
    for (int32_t k = 0; k < n1 && whole; k++) describe(k, 0, max_g);
    P.g_first = P.groups.size();
    for (int32_t k = n1; k < n_utt; k++) describe(k, 0, n_groups(P.order[k]));
    P.g_at.push_back(P.groups.size());
    const size_t n_rd = rd_f.size();
    P.g_lead = n_rd > 0 ? rd_g[1] : P.g_first;
    P.lead = n_rd > 0 ? rd_f[0] : 0;
    P.f_ready0 = n_rd > 1 ? rd_f[0] : n_rd == 1 ? INT32_MAX : 0;

    /* the script: the later rounds, *f_ready behind each; then the other takes' groups piece by piece, *q_ready following launch by launch
     * (the companion scores utterances faster than the first lanes decode them: a lane that is through with its utterance then finds the
     * next ones scored and stays -- with one step to n_utt at the end 239 of 256 lanes left and idled, profiles/r7_overlap_experiments.txt) */
    const auto score = [&](size_t a, size_t b) {
        for (size_t g = a; g < b; g += KFP_PIECE) P.script.push_back({ KFP_SCORE, (int64_t)g, (int64_t)std::min(g + KFP_PIECE, b) });
    };
    for (size_t r = 1; r < n_rd; r++) {
        score(rd_g[r], rd_g[r + 1]);
        P.script.push_back({ KFP_F_READY, r + 1 < n_rd ? rd_f[r] : INT32_MAX, 0 });
    }
    int32_t ready = n1;
    size_t g_end = P.g_first;           /* (the groups up to and with take `ready`: the table's tail is in take order) */
    for (size_t g = P.g_first; g < P.groups.size(); g += KFP_PIECE) {
        const size_t e = std::min(g + KFP_PIECE, P.groups.size());
        score(g, e);
        const int32_t was = ready;
        while (ready < n_utt && g_end + (size_t)n_groups(P.order[ready]) <= e) g_end += (size_t)n_groups(P.order[ready++]);
        if (ready > was) P.script.push_back({ KFP_Q_READY, ready, 0 });
    }
    if (ready < n_utt) P.script.push_back({ KFP_Q_READY, n_utt, 0 });
    return P;
}
#endif
