/* The schedule of the queue calls (cmusphinx_amd/csrc/s3a_qsched.h) under the host sanitizers, as a program of its own:
 *   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icmusphinx_amd/csrc tools/qsched_san.cpp -o /tmp/qsched_san && /tmp/qsched_san
 * The cases of tests/test_queue_events.py (a) .. (j) and seeded random ones through both builders; every array of every record is read
 * through (a checksum), and every event's lists are read at its offsets, so that a write or read out of bounds shows.  What the records
 * must BE is tests/test_queue_events.py's business. */
#include <stdio.h>
#include <stdlib.h>
#include "s3a_qsched.h"

static uint64_t sum = 0, records = 0;
static uint64_t rnd_x = 12345;
static uint32_t rnd() { rnd_x = rnd_x * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(rnd_x >> 33); }

static void
read_through(const QSched &Q)
{
    for (const std::vector<int32_t> *v : { &Q.lane, &Q.f0, &Q.epoch, &Q.last_utt, &Q.epoch_after, &Q.nfr_after, &Q.lists })
        for (int32_t x : *v) sum += (uint64_t)x;
    for (const QEvent &e : Q.events) {
        if (e.o_end < 0 || e.o_beg < e.o_end || (size_t)e.o_beg + 2 * (size_t)e.n_beg > Q.lists.size() || (size_t)e.o_end + 2 * (size_t)e.n_end > Q.lists.size()) {
            fprintf(stderr, "qsched_san: an event's lists lie outside the array\n");
            exit(1);
        }
        const int32_t *el = Q.lists.data() + e.o_end, *bl = Q.lists.data() + e.o_beg;
        for (int32_t i = 0; i < 2 * e.n_end; i++) sum += (uint64_t)el[i];
        for (int32_t i = 0; i < 2 * e.n_beg; i++) sum += (uint64_t)bl[i];
        sum += (uint64_t)(e.f + e.max_nfr);
    }
    sum += (uint64_t)Q.f_end;
    records++;
}

static void
run(const std::vector<int32_t> &n, int32_t n_lanes, int32_t boundary, const std::vector<int32_t> &epoch0 = {})
{
    const int32_t N = (int32_t)n.size();
    read_through(q_sched_refill(n_lanes, boundary, N, n.data(), epoch0.empty() ? NULL : epoch0.data()));
    read_through(q_sched_groups(kf_plan(N, n.data(), KFP_LANES, (size_t)n_lanes, false, 0, 0, 0, false), n.data(), n_lanes));
    read_through(QSched(N, std::min(n_lanes, N)));
}

int
main()
{
    const std::vector<int32_t> A = { 40, 8, 9, 1, 64, 17, 17, 33, 7, 16, 25, 3 };
    run(A, 4, 8); run(A, 4, 1); run(A, 3, 16); run(A, 40, 8); run(std::vector<int32_t>(16, 24), 4, 8); run({ 16, 17, 8, 9, 24, 1 }, 2, 8);
    run(A, 1, 8); run(A, 4, 8, { 1, 500, 0, 77 }); run(A, 8, 8);
    std::vector<int32_t> H;
    for (int i = 0; i < 1024; i++) H.push_back(300 + (int32_t)(rnd() % 2201));
    run(H, 256, 8);
    for (int t = 0; t < 400; t++) {
        std::vector<int32_t> n(1 + rnd() % 80);
        const int32_t top = t % 3 == 0 ? 9 : t % 3 == 1 ? 40 : 300, n_lanes = 1 + (int32_t)(rnd() % 24), boundary = 1 << (rnd() % 7);
        for (int32_t &v : n) v = 1 + (int32_t)(rnd() % top);
        std::vector<int32_t> e0;
        if (t % 2) for (int32_t z = 0; z < n_lanes; z++) e0.push_back((int32_t)(rnd() % (1u << 20)));
        run(n, n_lanes, boundary, e0);
    }
    /* refused: nothing but the empty record comes back */
    read_through(q_sched_refill(0, 8, 3, A.data(), NULL));
    read_through(q_sched_refill(4, 0, 3, A.data(), NULL));
    read_through(q_sched_refill(4, 8, 0, A.data(), NULL));
    const int32_t bad[3] = { 10, 0, 5 };
    read_through(q_sched_refill(4, 8, 3, bad, NULL));
    printf("qsched_san: %llu records, checksum %llu\n", (unsigned long long)records, (unsigned long long)sum);
    return 0;
}
