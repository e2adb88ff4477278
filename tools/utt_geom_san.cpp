/* The utterance engine's launch geometry (cmusphinx_amd/csrc/s3a_uttgeom.h) under the host sanitizers, as a program of its own:
 *   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icmusphinx_amd/csrc tools/utt_geom_san.cpp -o /tmp/utt_geom_san && /tmp/utt_geom_san
 * The cross product of tests/test_utt_geometry.py's inputs over three engine shapes, extreme shapes (one node, 2^30 nodes, no CUs, no
 * slots) and seeded random ones; every field of every record is read (a checksum).  The hazards: a division by zero, a signed overflow.
 * What the records must BE is tests/test_utt_geometry.py's business. */
#include <stdio.h>
#include <string.h>
#include "s3a_uttgeom.h"

static uint64_t sum = 0, records = 0;
static uint64_t rnd_x = 20261020;
static uint32_t rnd() { rnd_x = rnd_x * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(rnd_x >> 33); }
template <typename R> static void take(const R &r) { int32_t a[sizeof(R) / 4]; memcpy(a, &r, sizeof r); for (int32_t v : a) sum += (uint64_t)(int64_t)v; records++; }

static void
run(const UgShape &s, const UgCall &c, int32_t n, int32_t ov, int32_t slots, int64_t max_rows, int64_t budget)
{
    const UgEngine e = ug_engine(s);
    take(e); take(ug_frame(s, e, n, c.hist_sort_launch)); take(ug_score(s, ug_window_slots(e, n))); take(ug_score(s, slots));
    take(ug_companion(s, slots)); take(ug_kf(s, e, c, n, ov)); take(ug_score(s, 0)); take(ug_companion(s, 0));
    sum += (uint64_t)ug_route(s, e, c, max_rows, budget);
}

static UgShape
shape(int which)
{
    UgShape s;
    memset(&s, 0, sizeof s);
    s.n_emit = 3; s.nodepk = 1; s.D4 = UGC_D4MAIN; s.tab_size = 29350; s.tab16 = 1; s.max_cd = 100000; s.n_cu = 256; s.kf_slots = 512; s.kf_lds = 81376;
    s.big_wl = -1; s.window = -1; s.n_lanes = 512;
    switch (which) {
    case 0: s.N = 412; s.T = 2; s.maxn = 398; s.ent_cap = 40; s.n_pset = 150; s.n_sen = 602; s.n_ci_sen = 102; s.n_cs = 30; s.CP = 8; s.Gpad = 5120; s.gp_n = 16;
            s.maxhmmpf = 20000; s.hmmbeam = s.pbeam = -422133; break;
    case 1: s.N = 215748; s.T = 6; s.maxn = 71913; s.ent_cap = 192366; s.n_pset = 151038; s.n_sen = 6144; s.n_ci_sen = 144; s.n_cs = 12033; s.CP = 8; s.Gpad = 49152;
            s.gp_n = 188; s.tab_size = 29356; s.maxhmmpf = 20000; s.hmmbeam = -460586; s.pbeam = -383821; break;     /* (the bench engine's) */
    case 2: s.N = 412000; s.T = 4; s.maxn = 206000; s.ent_cap = 9000; s.n_pset = 60000; s.n_emit = 5; s.nodepk = 0; s.n_sen = 6138; s.n_ci_sen = 138; s.n_cs = 2200;
            s.CP = 32; s.Gpad = 196608; s.gp_n = 750; s.max_cd = 2000; s.maxhmmpf = 100000; s.hmmbeam = -767514; s.pbeam = -690762; s.ptranskip = 1; break;
    case 3: s.N = 1; s.T = 1; s.maxn = 1; s.ent_cap = 1; s.n_sen = 1; s.n_ci_sen = 1; s.CP = 1; s.Gpad = 512; s.n_cu = 0; s.kf_slots = 0; s.kf_lds = 0; s.n_lanes = 1; break;
    default: s.N = 1 << 30; s.T = UGC_WL_MAXT; s.maxn = 1 << 30; s.ent_cap = INT32_MAX; s.n_pset = 1 << 30; s.n_sen = INT32_MAX; s.n_ci_sen = 0; s.n_cs = INT32_MAX;
            s.CP = 64; s.Gpad = 1 << 30; s.gp_n = INT32_MAX; s.tab_size = INT32_MAX; s.maxhmmpf = INT32_MAX; s.hmmbeam = INT32_MIN; s.pbeam = INT32_MIN;
            s.n_cu = INT32_MAX; s.kf_slots = INT32_MAX; s.kf_lds = INT32_MAX; s.n_lanes = 1024; break;
    }
    return s;
}

int
main()
{
    const int32_t lanes[] = { 1, 7, 8, 9, 16, 17, 31, 32, 63, 64, 95, 96, 128, 255, 256, 257, 512, 1024 }, totals[] = { 8, 16, 64, 1024, 4096, 8184 };
    for (int w = 0; w < 5; w++) for (int32_t n : lanes) for (int32_t slots : { 256, 512 }) for (int32_t alone = 0; alone < 2; alone++) for (int32_t cluster : { 0, 2, 3 })
        for (int32_t relay_at : { 0, 4 }) for (int32_t persist = -1; persist <= 2; persist++) for (int32_t window = -1; window <= 0; window++)
            for (int32_t pheur = 0; pheur < 2; pheur++) for (int32_t sp = 0; sp < 2; sp++) {
                UgShape s = shape(w);
                UgCall c;
                memset(&c, 0, sizeof c);
                if (w < 3) s.kf_slots = slots;
                s.n_lanes = std::max(n, w == 3 ? 1 : 8); s.cluster = cluster; s.persist = persist; s.window = window; s.pheurtype = pheur;
                c.alone = alone; c.kf_relay_at = relay_at; c.second_pass = sp; c.queue = (n + sp) & 1; c.n_utt = c.queue ? 2 * n + 1 : n;
                run(s, c, std::min(n, s.n_lanes), pheur, totals[(n + slots / 256 + cluster) % 6], sp ? 1 : 0, alone ? INT64_MAX : 0);
            }
    for (int t = 0; t < 20000; t++) {
        UgShape s = shape((int)(rnd() % 5));
        UgCall c;
        int32_t *sv = (int32_t *)&s, *cv = (int32_t *)&c;
        for (size_t i = 0; i < sizeof c / 4; i++) cv[i] = rnd() % 4 == 0 ? (int32_t)(rnd() % 2000) - 4 : 0;
        for (int k = 0; k < 3; k++) {       /* a few fields of the shape at random, extremes among them */
            const uint32_t r = rnd() % 8;
            sv[rnd() % (sizeof s / 4)] = r == 0 ? INT32_MAX : r == 1 ? INT32_MIN : r == 2 ? 0 : r == 3 ? -1 : (int32_t)(rnd() % 100000);
        }
        /* (what every caller guarantees: s3a_uttdec_init's argument checks, s3a_utt_geometry's) */
        s.n_lanes = 1 + (int32_t)(rnd() % 1024); s.T = 1 + (int32_t)(rnd() % UGC_WL_MAXT); s.CP = 1 << (rnd() % 7);
        s.N = std::max(s.N, 0) & 0x3fffffff; s.maxn = std::max(s.maxn, 0) & 0x3fffffff; s.ent_cap = std::max(s.ent_cap, 0); s.Gpad = std::max(s.Gpad, 0) & ~511;
        s.n_ci_sen = std::max(0, std::min(s.n_ci_sen, 1 << 20)); s.n_sen = std::max(s.n_sen, s.n_ci_sen); s.n_cs = std::max(s.n_cs, 0); s.tab_size = std::max(s.tab_size, 0);
        s.n_cu = std::max(s.n_cu, 0); s.kf_slots = std::max(s.kf_slots, 0); s.hmmbeam = std::min(s.hmmbeam, 0); s.pbeam = std::min(s.pbeam, 0);
        s.maxhmmpf = std::max(s.maxhmmpf, 0); s.gp_n = std::max(s.gp_n, 0);
        c.n_utt = 1 + (int32_t)(rnd() % 4096); c.kf_relay_at = std::max(c.kf_relay_at, 0); c.kf_overlap_round = std::max(c.kf_overlap_round, 0);
        const int32_t n = 1 + (int32_t)(rnd() % s.n_lanes);
        run(s, c, n, (int32_t)(rnd() % 2), 1 + (int32_t)(rnd() % 20000), (int64_t)(rnd() % 3), (int64_t)(rnd() % 3));
    }
    printf("utt_geom_san: %llu records, checksum %llu\n", (unsigned long long)records, (unsigned long long)sum);
    return 0;
}
