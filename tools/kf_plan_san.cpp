/* The plan of the ku_frames calls (cmusphinx_amd/csrc/s3a_kfplan.h) under the host sanitizers, as a program of its own:
 *   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icmusphinx_amd/csrc tools/kf_plan_san.cpp -o /tmp/kf_plan_san && /tmp/kf_plan_san
 * The cases of tests/test_kf_plan.py (a) .. (i) and seeded random ones; every array of every plan is read through (a checksum), so that a
 * write or read out of bounds inside kf_plan shows.  What the plans must BE is tests/test_kf_plan.py's business. */
#include <stdio.h>
#include "s3a_kfplan.h"

static uint64_t sum = 0, plans = 0;
static uint64_t rnd_x = 12345;
static uint32_t rnd() { rnd_x = rnd_x * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(rnd_x >> 33); }

static void
run(const std::vector<int32_t> &n, int32_t rule, size_t budget, bool in_order, int32_t n1, int32_t lead_g, int32_t round_g, bool whole)
{
    const KfPlan P = kf_plan((int32_t)n.size(), n.data(), rule, budget, in_order, n1, lead_g, round_g, whole);
    for (int32_t v : P.order) sum += (uint64_t)v;
    for (int32_t v : P.cut) sum += (uint64_t)v;
    for (int64_t v : P.row0) sum += (uint64_t)v;
    for (size_t v : P.g_at) sum += v;
    for (const KfGroup &g : P.groups) sum += (uint64_t)(g.utt + g.first + g.frames) + (uint64_t)g.row;
    for (const KfStep &s : P.script) sum += (uint64_t)(s.op + s.a + s.b);
    sum += P.max_rows + P.g_first + P.g_lead + (uint64_t)P.n1 + (uint64_t)P.lead + (uint64_t)P.f_ready0;
    plans++;
}

int
main()
{
    const std::vector<int32_t> A = { 40, 8, 9, 1, 64, 17, 17, 33, 7, 16, 25, 3 };
    const size_t BIG = (size_t)1 << 40;
    run(A, KFP_BUDGET, BIG, false, 4, 1, 1, false);
    run(A, KFP_BUDGET, BIG, false, 4, 1, 1, true);
    run(A, KFP_BUDGET, BIG, true, 4, 1, 1, false);
    run(std::vector<int32_t>(16, 24), KFP_BUDGET, BIG, false, 4, 1, 1, false);
    run({ 5, 3, 7, 2, 6, 4, 1, 3, 5, 2 }, KFP_BUDGET, BIG, false, 3, 2, 1, false);
    std::vector<int32_t> F, I;
    for (int i = 0; i < 20; i++) F.push_back(10 + (i * 37) % 53);
    run(F, KFP_BUDGET, 300, false, 0, 0, 0, false);
    run(A, KFP_LANES, 8, false, 0, 0, 0, false);
    run({ 12, 30, 8, 1, 17 }, KFP_ONE, 0, true, 0, 0, 0, false);
    for (int i = 0; i < 1024; i++) I.push_back(300 + (int32_t)(rnd() % 2201));
    run(I, KFP_BUDGET, BIG, false, 256, 16, 4, false);
    for (int t = 0; t < 400; t++) {
        std::vector<int32_t> n(1 + rnd() % 60);
        const int32_t top = t % 3 == 0 ? 9 : t % 3 == 1 ? 40 : 300;
        for (int32_t &v : n) v = 1 + (int32_t)(rnd() % top);
        const int32_t rule = (int32_t)(rnd() % 3);
        const size_t budget = rule == KFP_LANES ? 1 + rnd() % 20 : rnd() % 2 ? BIG : 1 + rnd() % 400;
        run(n, rule, budget, rnd() % 2 != 0, (int32_t)(rnd() % (n.size() + 2)), (int32_t)(rnd() % 6), (int32_t)(rnd() % 4), t % 5 == 0);
    }
    printf("kf_plan_san: %llu plans, checksum %llu\n", (unsigned long long)plans, (unsigned long long)sum);
    return 0;
}
