/* The utterance engine's LAUNCH GEOMETRY (s3a_utt.hip), as data: grid sizes, workgroups per lane, the kernel variant taken from a given lane
 * count on, the LDS of a scoring workgroup, ku_frames' cluster sizes and relay stages, and what a call runs as -- arithmetic on a handful of
 * integers, no device and no engine types, so that it can be stated and checked without a GPU (s3a_utt_geometry, tests/test_utt_geometry.py,
 * tools/utt_geom_san.cpp).  The engine computes these records and launches from them; nothing here is recomputed beside a launch.
 *
 * Conventions.  Every record is a struct of int32_t fields ONLY, declared through a field list (UG_*_FIELDS): the same list names the
 * fields for the hooks, so a record is also an int32_t array in that order.  Flags are 0 / 1.  A grid is workgroups in x; y and z are said
 * where they are not (1, lanes).  `n` is the lanes a launch keeps busy, `n_lanes` the engine's.  A record holds CHOICES (threads 256 or 1024,
 * a variant's number) and sizes, never function pointers: the caller's ladder over template instantiations reads them.
 *   UgShape   what the rules read: the lextree, the model, the search configuration, the device, the engine, the options
 *   UgCall    what a call adds: its kind and size, what else runs on the device, the process-wide variants in force
 *   UgEngine  fixed at init              ug_engine(shape)
 *   UgFrame   per lanes of a call        ug_frame(shape, engine, n, hist_sort_launch)
 *   UgScore   a look-ahead scoring pass  ug_score(shape, slots) | ug_companion(shape, slots): the shape that fits beside ku_frames
 *   UgKf      a ku_frames call           ug_kf(shape, engine, call, n, ov)
 *   route     what a call runs as        ug_route(shape, engine, call, max_rows, budget) */
#ifndef S3A_UTTGEOM_H
#define S3A_UTTGEOM_H
#include <stdint.h>
#include <algorithm>

/* ---- constants the kernels use too: copies (s3a_utt.hip holds each to the kernels' own with a static_assert) ---- */
enum {
    UGC_DBLOCK = 256, UGC_RSBLOCK = 64, UGC_M3BLOCK = 64, UGC_SCAN_THREADS = 1024, UGC_UR_K = 8, UGC_UW_FB = 8, UGC_USEL_G = 8, UGC_UG_FB = 8,
    UGC_UG_MAX = 32, UGC_WL_THREADS = 512, UGC_WL_MAXT = 16, UGC_WL_MAXCALL = 96, UGC_WL_BIG_G = 256, UGC_UE_WG_PER_TREE = 16, UGC_KF_MAXC = 32,
    UGC_KF_SENBITS = 16384, UGC_KF_STAGES = 2, UGC_KF_LEAD = 128, UGC_PIECE = 1024, UGC_D4MAIN = 10, UGC_EVBLOCK_LONG_LIST = 32768,
    UGC_SCAN_LONG_LIST = 16384, UGC_UWGROUP_BYTES = 32,
    UGC_CU_LDS = 160 * 1024             /* LDS of a CU; a workgroup's allocation granule there is 1 280 B (512 B on the older parts) */
};

/* ---- the tuned constants: each with the measurement it came from ---- */
/* fixed grids, sized for the usual frame: a workgroup loops when a list is longer (virtual workgroups); with many lanes the idle workgroups
 * of a generous grid cost more than the loop */
/* (many lanes: NOT a multiple of 16 -- measured with four 128-lane engines: 32 / 48 / 64 / 96 workgroups per (tree, lane) 406 / 424 / 411 /
 * 409 k frames/s, 24 ... 72 otherwise 428 ... 438 k, odd counts best: consecutive (tree, lane) groups then start on rotating XCDs instead of
 * piling every group's first, always busy, workgroup onto the same one) */
static constexpr int32_t UGT_G_EVAL_MANY = 57;
static constexpr int32_t UGT_G_RES_MANY = 49; /* (128: 401 k, 96: 403 k, 64: 405 k / 408.5 k, 48: 411 k, 32: 410 k frames/s; + UGT_UR_GL an odd total) */
/* (wide beams keep the round-3 SWEEP in the resolve launch, whose workgroups UGT_G_RES_MANY was never meant to size: 128 there, as before the
 * list-position grids were retuned -- configs[4]: 363 us per launch against 659) */
static constexpr int32_t UGT_G_RES_WIDE = 128;
static constexpr int32_t UGT_G_ENT = 256;
static constexpr int32_t UGT_G_MARK_MANY = 128; /* (many lanes: 1024 workgroups per lane were 131 k per launch, most of them idle: 50 -> 30 us per 128-lane launch, 331 -> 349 k frames/s) */
static constexpr int32_t UGT_G_ENTER2_MANY = 12; /* ku_enter2's workgroups per lane with many lanes (they take the calls in turn) */
static constexpr int32_t UGT_G_HIST_MANY = 9; /* ku_hist_count's workgroups per (tree, lane) with many lanes (5: 440.1, 7: 445.1, 8: 440.4, 9: 447.5 k frames/s) */
static constexpr int32_t UGT_UR_GL = 192;   /* one-wave workgroups per lane that walk the listed sets (one box: 128: 353.5 k, 256: 362.2 k, 512: 363.9 k frames/s; the sweep: 355.9 k) */
static constexpr int32_t UGT_UG_MANY = 32;  /* lanes from which the grids / kernels for many lanes per launch are used (s3a_uttdec_opts_t.many) */
/* from this many lanes on, 256-thread workgroups for ku_enter2, the histogram sort and the one-workgroup-per-tree scan
 * (s3a_uttdec_opts_t.scan_small_from).  ku_enter2: 365 -> 371 k frames/s with four engines on the chip.  The scan: four times the chunks to
 * walk, 53 instead of 29 us per 128-lane launch alone, but with four engines on the chip a 256-thread workgroup finds a slot where a
 * 1024-thread one waits for half a CU: 355 -> 362 k frames/s; with 32-lane engines the other way round: 268 -> 259 k.  The sort: the launch's
 * workgroups mostly only leave, and small ones find a slot sooner */
static constexpr int32_t UGT_UG_SCAN_SMALL = 64;
static constexpr int32_t UGT_UG_SCAN_CHAIN_MAX = 768; /* the chained scan (a workgroup per chunk) when that is no more workgroups than the chip holds: a single lane, wide beams */
static constexpr int32_t UGT_UG_WIDE_BEAM = 50000; /* -maxhmmpf and the largest tree from which the word level's candidate phases are launches of their own */
/* ku_frames pays from UGT_KF_MIN_LANES lanes on.  Measured with one engine on the hub4-shaped task, ku_frames : launches, k frames/s -- 256 lanes
 * 443 : 288, 128 lanes (clusters of 3) 407 : 223, 64 lanes (4) 273 : 153, 32 lanes (4) 159 : 110, 16 lanes (8) 91 : 73, 8 lanes (8)
 * 54.7 : 45.2, 4 lanes (16) 28.2 : 27.7, one lane (16) 7.6 : 9.4 -- with the clusters' XCD-local barrier (the general one, an L2
 * write-back per workgroup and step: 128 lanes 284, 64 lanes 216, and the launches won below 96 lanes).  Larger clusters do not pay
 * (32 lanes: 159 / 146 / 94 k with 4 / 8 / 15 workgroups; 64 lanes: 273 / 219 k with 4 / 7): the entry ranking and the word level
 * stay one workgroup's */
static constexpr int32_t UGT_KF_MIN_LANES = 8;
static inline int32_t ug_kf_cluster_max(int32_t n) { return n <= 16 ? 8 : 4; }
static constexpr int32_t UGT_KF_CLUSTER_MAX_WIDE = 8; /* (wide beams: seven times the HMMs, a word level in chunks) */
/* a cluster's workgroups spin on one another, so a grid must never exceed what is resident; the occupancy query the slots come from can be
 * one workgroup per CU high (MI355X_MICROARCH "Residency and cooperative launch"): of an XCD's slots, when there are more than 8, 4 stay free */
static constexpr int32_t UGT_KF_XCD_MARGIN = 4;
static constexpr int32_t UGT_UW_COMP_FPC_MAX = 88; /* frames per chunk of the companion scoring shape at most (what fits beside the table and the tile) */

/* ---- the records ---- */
#define UG_SHAPE_FIELDS(X) \
    X(N) X(T) X(maxn) X(ent_cap) X(n_pset) X(n_emit) X(nodepk)                  /* lextree: nodes, trees, the largest tree's nodes, entry capacity */ \
    X(n_sen) X(n_ci_sen) X(n_cs) X(CP) X(D4) X(Gpad) X(gp_n) X(tab_size) X(max_cd) X(tab16) /* model (tab16: the 16-bit log-add table exists) */ \
    X(maxhmmpf) X(hmmbeam) X(pbeam) X(ptranskip) X(pheurtype)                   /* search configuration */ \
    X(n_cu) X(kf_slots) X(kf_lds)       /* device: CUs | occupancy x CUs and static LDS of the ku_frames instantiation this engine launches (0: not asked) */ \
    X(n_lanes) X(exact)                                                         /* engine */ \
    X(many) X(big_wl) X(window) X(scan_small_from) X(persist) X(cluster) X(graph) X(framecheck)    /* s3a_uttdec_opts_t, as given */
#define UG_CALL_FIELDS(X) \
    X(queue) X(n_utt)                   /* s3a_uttdec_decode_queue (else s3a_uttdec_decode) | its utterances */ \
    X(alone)                            /* the engine may size clusters for the whole device (no other engine, no other process's lock) */ \
    X(prof_every) X(second_pass) X(keep_lat)    /* per-launch profiling on | the second pass is enabled | ... and its lattices are kept */ \
    X(hist_sort_launch) X(kf_no_relay) X(kf_relay_at) X(kf_no_overlap) X(kf_overlap_n1) X(kf_overlap_lead) X(kf_overlap_round)  /* s3a_variants_t */
#define UG_ENGINE_FIELDS(X) \
    X(eval_block) X(g_eval) X(g_res) X(g_ent) X(g_mark) /* ku_hmm_eval's threads and workgroups per (tree, lane) | per lane: resolve (list part), enter1, enter3 */ \
    X(scan_nc)                          /* chunks of the scan over a tree's list */ \
    X(hist_possible) X(weak_possible) X(big_wl) \
    X(win_K) X(many) X(scan_small_from) X(use_graph) \
    X(persist)                          /* 0: never ku_frames | 1: where it pays | 2: whatever the lane count | 3: and with the general barrier only */
enum { UG_RES_PLIST = 0, UG_RES_LISTS = 1, UG_RES_SWEEP = 2 };
#define UG_FRAME_FIELDS(X) \
    X(n) \
    X(enter2_threads) X(g_enter2) \
    X(g_ci) X(g_cd) X(g_cs) X(g_sel) X(dyn_ci)  /* 256-thread workgroups over the CI / CD / composite senones, ku_select's | -maxcdsenpf: ku_dyn_ci_beam */ \
    X(multi) X(gm_x) X(gm_y) X(gm_z)    /* per-frame scoring (win_K = 0): the CD senones of all lanes as one pass, its grid */ \
    X(by_parents)                       /* the not active nodes from the list of stamped parent sets (not with wide beams: faster with the sweep) */ \
    X(own_sort) X(g_hist) X(sort_threads)       /* the histogram sort rides on the count's launch | the count's grid x | the sort's own launch */ \
    X(resolve) X(g_resolve) X(GB)       /* UG_RES_* | its grid | workgroups of the sweep's part */ \
    X(scan_gc) X(scan_threads) X(g_scan) X(scan_nc_arg)  /* workgroups per tree (1 or scan_nc) | 256: ku_scan<256> | grid | the kernel's chunk argument */ \
    X(g_emit) X(g_wide)                 /* ku_emit_word | the wide-beam word level's launches (0: none) */
#define UG_SCORE_FIELDS(X) \
    X(nt) X(fpc) X(n_chunks) X(n_tiles) X(grid) X(tab_lds) X(lds)       /* threads | (lane, frame) slots per chunk | ... | the table in LDS | dynamic LDS bytes */
#define UG_KF_FIELDS(X) \
    X(served)                           /* this engine, as it is configured now, runs n lanes' frames through ku_frames */ \
    X(usable)                           /* workgroups of ku_frames an XCD holds at once, less the margin */ \
    X(C) X(grid)                        /* workgroups per lane of a single launch (KF_WINDOW blocks) | its grid */ \
    X(c0) X(grid0)                      /* the same for a chain's first launch */ \
    X(n_st) X(st_c1) X(st_cap1) X(st_grid1) X(st_c2) X(st_cap2) X(st_grid2)     /* the relay's stages: cluster size, lanes at most, grid */ \
    X(n1) X(lead_g) X(round_g)          /* KF_QUEUE: first lanes of a call scored beside the search (0: none) | groups of the lead, of a round */
#define UG_DECL(f) int32_t f;
#define UG_NAME(f) #f ","
struct UgShape { UG_SHAPE_FIELDS(UG_DECL) };
struct UgCall { UG_CALL_FIELDS(UG_DECL) };
struct UgEngine { UG_ENGINE_FIELDS(UG_DECL) };
struct UgFrame { UG_FRAME_FIELDS(UG_DECL) };
struct UgScore { UG_SCORE_FIELDS(UG_DECL) };
struct UgKf { UG_KF_FIELDS(UG_DECL) };
enum { UG_REC_SHAPE = 0, UG_REC_CALL, UG_REC_ENGINE, UG_REC_FRAME, UG_REC_SCORE, UG_REC_KF, UG_REC_N };
static inline const char *
ug_field_names(int32_t rec)
{
    switch (rec) {
    case UG_REC_SHAPE: return UG_SHAPE_FIELDS(UG_NAME);
    case UG_REC_CALL: return UG_CALL_FIELDS(UG_NAME);
    case UG_REC_ENGINE: return UG_ENGINE_FIELDS(UG_NAME);
    case UG_REC_FRAME: return UG_FRAME_FIELDS(UG_NAME);
    case UG_REC_SCORE: return UG_SCORE_FIELDS(UG_NAME);
    case UG_REC_KF: return UG_KF_FIELDS(UG_NAME);
    default: return "";
    }
}
#undef UG_DECL
#undef UG_NAME

/* what a call runs as */
enum {
    UG_ROUTE_GRAPH = 0,     /* blocks of frames replayed as a HIP graph */
    UG_ROUTE_KF_STATIC,     /* every frame scored first, then lane z = utterance z as one chain of ku_frames launches */
    UG_ROUTE_KF_QUEUE,      /* ... the lanes take the queue's utterances themselves */
    UG_ROUTE_KF_GROUPS,     /* the second-pass / -pheurtype queue: groups of at most n_lanes utterances, each a KF_STATIC launch */
    UG_ROUTE_WINDOW,        /* window blocks: a scoring pass + one ku_frames launch per look-ahead window */
    UG_ROUTE_FRAMES         /* the frame as a dozen launches */
};

static inline int32_t ug_ceil(int64_t a, int64_t b) { return (int32_t)((a + b - 1) / b); }
static inline int32_t ug_i32(int64_t v) { return (int32_t)std::min<int64_t>(v, INT32_MAX); }

/* ---- the engine's geometry, once at init ---- */
static inline UgEngine
ug_engine(const UgShape &s)
{
    using std::max; using std::min;
    UgEngine e;
    e.eval_block = (s.maxhmmpf >= UGC_EVBLOCK_LONG_LIST && s.maxn >= UGC_EVBLOCK_LONG_LIST) ? 256 : 64;
    e.many = s.many > 0 ? s.many : UGT_UG_MANY;
    const bool many = s.n_lanes >= e.many;
    /* wide beams (thousands of word exits, 10^5..10^6 (exit, predecessor) candidates per frame): the word level's candidate phases run
     * chip-wide as their own launches; opts->big_wl = 0 / 1 overrides */
    e.big_wl = s.big_wl >= 0 ? (s.big_wl != 0) : (s.maxhmmpf >= UGT_UG_WIDE_BEAM && s.maxn >= UGT_UG_WIDE_BEAM);
    e.g_eval = max(1, min(ug_ceil(s.maxn, e.eval_block), many ? UGT_G_EVAL_MANY : 2048 / max(1, min(s.n_lanes, 8))));
    e.g_res = max(1, min(ug_ceil(s.N, UGC_RSBLOCK), many ? (e.big_wl ? UGT_G_RES_WIDE : UGT_G_RES_MANY) : 1024));
    e.g_ent = max(1, min(ug_ceil(s.ent_cap, 256), UGT_G_ENT));
    e.g_mark = (int32_t)max<int64_t>(1, min<int64_t>((int64_t)ug_ceil(s.ent_cap, UGC_M3BLOCK) + (int64_t)ug_ceil(s.maxn, UGC_M3BLOCK) * s.T, 1024));
    if (many) e.g_mark = min(e.g_mark, UGT_G_MARK_MANY);
    e.scan_nc = (s.maxhmmpf >= UGC_SCAN_LONG_LIST && s.maxn >= UGC_SCAN_LONG_LIST) ? ug_ceil(s.maxn, UGC_SCAN_THREADS) : 1;
    /* lextree_hmm_histbin can only fire when more than 1.5 x maxhmmpf HMMs can be active at all */
    e.hist_possible = (int64_t)s.N > (int64_t)s.maxhmmpf + (s.maxhmmpf >> 1);
    e.weak_possible = s.ptranskip != 0 || s.pbeam < s.hmmbeam;
    /* look-ahead scoring (ku_score_window): the 39/40-dimensional case with a 16-bit log-add table and at most 64 Gaussian slots per
     * senone; K = 8 frames per window: from 128 lanes on that is the ~1024 (lane, frame) slots a model pass amortises over, and with fewer
     * lanes a longer window buys < 1 % (measured: one lane 94.6 x real time with K = 64, 93.5 with 8; 8 and 32 lanes: no difference) while a
     * refilled lane has to wait for a window boundary.  opts->window: exactly that many frames (0: the per-frame scoring kernels). */
    e.win_K = 0;
    if (s.tab16 && s.D4 == UGC_D4MAIN && s.CP <= 64 && s.Gpad % 512 == 0) e.win_K = s.window >= 0 ? ug_i32((int64_t)ug_ceil(s.window, 8) * 8) : 8;
    e.scan_small_from = s.scan_small_from > 0 ? s.scan_small_from : UGT_UG_SCAN_SMALL;
    e.use_graph = s.graph != 0 && !e.big_wl && !s.framecheck;
    e.persist = s.persist >= 0 && !e.use_graph && !s.framecheck ? (s.persist > 1 ? 3 : s.persist > 0 ? 2 : 1) : 0;
    return e;
}

/* ---- a frame's launches for n lanes ---- */
static inline UgFrame
ug_frame(const UgShape &s, const UgEngine &e, int32_t n, int32_t hist_sort_launch)
{
    using std::max; using std::min;
    UgFrame g;
    const bool many = n >= e.many, small = n >= e.scan_small_from;
    g.n = n;
    g.enter2_threads = small ? 256 : UGC_SCAN_THREADS;
    g.g_enter2 = small || many ? UGT_G_ENTER2_MANY : UGC_WL_MAXCALL;
    g.g_ci = ug_ceil((int64_t)s.n_ci_sen * s.CP, 256);
    g.g_cd = ug_ceil((int64_t)(s.n_sen - s.n_ci_sen) * s.CP, 256);
    g.g_cs = ug_ceil(s.n_cs, 256);              /* composite senones: a wave looks at 64 */
    g.g_sel = max(1, min((int32_t)UGC_USEL_G, min(s.gp_n, ug_ceil(s.n_sen - s.n_ci_sen, 256))));
    g.dyn_ci = s.max_cd < s.n_sen - s.n_ci_sen;
    /* per-frame scoring: from UG_FB lanes on the CD senones of all lanes are ONE pass over the model (39/40-dimensional features, >= UG_FB
     * Gaussian slots per senone) */
    g.multi = e.win_K == 0 && n >= UGC_UG_FB && s.D4 == UGC_D4MAIN && s.CP >= UGC_UG_FB && s.CP <= 64 && g.g_cd > 0 && s.gp_n == g.g_cd;
    g.gm_x = g.g_cd; g.gm_z = ug_ceil(n, UGC_UG_MAX);
    g.gm_y = (int32_t)max<int64_t>(1, min<int64_t>(ug_ceil(min(n, (int32_t)UGC_UG_MAX), UGC_UG_FB), 2 * (int64_t)s.n_cu / max<int64_t>(1, (int64_t)g.g_cd * g.gm_z)));
    g.by_parents = many && !e.big_wl;
    /* many lanes: the (rare) histogram sort rides on the count's launch (its 256-thread form is the one used there anyway) */
    g.own_sort = e.hist_possible && small && !hist_sort_launch;
    g.g_hist = max(1, min(ug_ceil(s.maxn, UGC_DBLOCK), many ? UGT_G_HIST_MANY : 64));
    g.sort_threads = small ? 256 : UGC_SCAN_THREADS;
    /* (the active HMMs by list position: g_res workgroups that loop; the rest: the listed sets, or a sweep, UR_K nodes per thread) */
    g.GB = ug_ceil(ug_ceil(s.N, UGC_UR_K), UGC_RSBLOCK);
    g.resolve = g.by_parents ? UG_RES_PLIST : many ? UG_RES_LISTS : UG_RES_SWEEP;
    g.g_resolve = g.by_parents ? e.g_res + UGT_UR_GL : many ? ug_i32((int64_t)e.g_res + g.GB) : ug_ceil(s.N, UGC_RSBLOCK);
    /* the scan over long lists: either one workgroup per possible chunk, chained (a chunk waits for chunks with SMALLER numbers only =
     * workgroups dispatched before it: the wait ends whatever else runs on the chip), when that is no more workgroups than the chip holds, or
     * one workgroup per tree that walks the chunks itself with the totals in a register -- no flags, no look-back.  (A few workgroups per tree
     * taking the chunks in turn is NOT an option: workgroup 0's second chunk then waits for the LAST workgroup's first, a workgroup dispatched
     * after it -- with several engines on the chip every slot can end up held by such a waiter: WL_E_SCAN time-outs with 8 engines of 64 lanes) */
    g.scan_gc = (int64_t)s.T * n * e.scan_nc <= UGT_UG_SCAN_CHAIN_MAX ? e.scan_nc : 1;
    g.scan_threads = g.scan_gc == 1 && small ? 256 : UGC_SCAN_THREADS;
    g.g_scan = s.T * g.scan_gc;
    g.scan_nc_arg = g.scan_gc == 1 ? 1 : e.scan_nc;
    /* (many lanes: fewer emission workgroups per tree -- each sweeps further -- instead of thousands of idle ones) */
    g.g_emit = 1 + (many && !e.big_wl ? 1024 / UGC_WL_THREADS : UGC_UE_WG_PER_TREE) * s.T;
    g.g_wide = e.big_wl ? UGC_WL_BIG_G : 0;
    return g;
}

/* ---- look-ahead scoring: ku_score_window's shape ---- */
/* (lane, frame) slots of the pass that scores n lanes' coming window */
static inline int32_t ug_window_slots(const UgEngine &e, int32_t n) { return std::max(1, ug_i32((int64_t)n * e.win_K)); }

static inline int32_t
ug_score_lds(int32_t fpc, int32_t nt, bool tab_lds, int32_t tab_size)
{
    int64_t b = (int64_t)fpc * UGC_D4MAIN * 4 * 4;                      /* the chunk's features */
    b += (int64_t)(nt / 64) * UGC_UW_FB * 65 * 4;                       /* the waves' transposition tiles */
    b = (b + 15) & ~(int64_t)15;
    b += (int64_t)(fpc / UGC_UW_FB) * UGC_UWGROUP_BYTES;
    b = (b + 15) & ~(int64_t)15;
    if (tab_lds) b += ((int64_t)tab_size * 2 + 15) & ~(int64_t)15;
    return ug_i32(b);
}

/* `total` (lane, frame) slots (fewer than one: taken as one).  Slots per chunk: a workgroup needs ~100 KB of LDS, so one is resident per CU and the grid runs in
 * rounds of n_cu workgroups; time ~ rounds x (slots per chunk + a start-up worth ~10 slots) */
static inline UgScore
ug_score(const UgShape &s, int32_t total)
{
    const int32_t n_cu = std::max(1, s.n_cu);
    UgScore q;
    total = std::max(total, 1);
    q.tab_lds = total >= 2 * UGC_UW_FB ? 1 : 0;
    q.nt = q.tab_lds ? 512 : 256;
    q.n_tiles = s.Gpad / q.nt;
    q.fpc = UGC_UW_FB;
    int64_t best_cost = -1;
    for (int32_t nc = 1; nc <= 512; nc++) {
        const int64_t fpc64 = (int64_t)ug_ceil(ug_ceil(total, nc), UGC_UW_FB) * UGC_UW_FB;
        if (fpc64 > 256) continue;
        const int32_t fpc = (int32_t)fpc64;
        const int64_t rounds = ((int64_t)q.n_tiles * ug_ceil(total, fpc) + n_cu - 1) / n_cu, cost = rounds * (fpc + 10);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; q.fpc = fpc; }
        if (fpc <= UGC_UW_FB) break;
    }
    q.n_chunks = ug_ceil(total, q.fpc);
    q.grid = ug_i32((int64_t)ug_ceil(q.n_tiles, 8) * q.n_chunks * 8);
    q.lds = ug_score_lds(q.fpc, q.nt, q.tab_lds != 0, s.tab_size);
    if (q.lds > UGC_CU_LDS) { q.tab_lds = 0; q.lds = ug_score_lds(q.fpc, q.nt, false, s.tab_size); }
    return q;
}

/* THE COMPANION SHAPE: a scoring workgroup that fits a CU BESIDE one ku_frames workgroup (a queue's later utterances are scored while the
 * first ones are searched).  256 threads at no more than 256 VGPRs are one wave per SIMD beside the search's two of 128; the LDS is what the
 * CU has left beside the search's workgroup, by that kernel's own figure (ku_frames' static LDS rounded up to the allocation granule,
 * 1 280 B on a 160 KB CU -- and to 512 B, the older parts', whichever leaves less): the log-add table, the transposition tile and as many
 * frames per chunk as still fit (at most UGT_UW_COMP_FPC_MAX).  Same body, same rows as every other shape. */
static inline int32_t
ug_companion_room(int32_t kf_lds)
{
    int32_t lane = kf_lds;
    if (lane <= 0 || lane > UGC_CU_LDS / 2) lane = UGC_CU_LDS / 2;
    const int32_t left = UGC_CU_LDS - std::max((lane + 1279) / 1280 * 1280, (lane + 511) / 512 * 512);
    return left / 1280 * 1280;
}
static inline UgScore
ug_companion(const UgShape &s, int32_t total)
{
    total = std::max(total, 1);
    const int32_t room = ug_companion_room(s.kf_lds), fpc0 = (int32_t)std::min<int64_t>(UGT_UW_COMP_FPC_MAX, (int64_t)ug_ceil(total, UGC_UW_FB) * UGC_UW_FB);
    UgScore q;
    q.nt = 256; q.tab_lds = 1;
    q.n_tiles = s.Gpad / q.nt;
    q.fpc = fpc0;
    while (q.fpc > UGC_UW_FB && ug_score_lds(q.fpc, q.nt, true, s.tab_size) > room) q.fpc -= UGC_UW_FB;
    if (ug_score_lds(q.fpc, q.nt, true, s.tab_size) > room) { q.tab_lds = 0; q.fpc = fpc0; }   /* (a table that does not fit beside the search stays in memory) */
    q.n_chunks = ug_ceil(total, q.fpc);
    q.grid = ug_i32((int64_t)ug_ceil(q.n_tiles, 8) * q.n_chunks * 8);
    q.lds = ug_score_lds(q.fpc, q.nt, q.tab_lds != 0, s.tab_size);
    return q;
}

/* ---- ku_frames ---- */
/* does this engine, as it is configured now, run n lanes' frames through ku_frames?  NOT served: an engine without look-ahead scoring
 * (win_K = 0), with per-launch profiling on, graph replay or the frame check (persist = 0), 3-state HMMs without the packed node records,
 * more senones than KF_SENBITS; and, unless asked for (persist > 1), fewer than UGT_KF_MIN_LANES lanes or a wide-beam engine -- that one is
 * served, word level and all, but keeps the launches: 23 000 HMMs and 300 000 word-level candidates per lane-frame want the whole chip per
 * step, not a cluster of 8 workgroups (64 lanes: 10.4 k frames/s through ku_frames against 30.5 k through the launches, 128 lanes 19.4 k :
 * 36.1 k; profiles/r6_experiments.txt 8) */
static inline bool
ug_kf_served(const UgShape &s, const UgEngine &e, const UgCall &c, int32_t n)
{
    return e.persist && (e.persist > 1 || (n >= UGT_KF_MIN_LANES && !e.big_wl)) && e.win_K > 0 && c.prof_every == 0
        && ((s.n_emit == 3 && s.nodepk) || s.n_emit == 5) && s.T <= UGC_WL_MAXT && s.n_sen <= UGC_KF_SENBITS;
}

/* workgroups of ku_frames an XCD holds at once, less the margin */
static inline int32_t
ug_kf_usable(const UgShape &s)
{
    const int32_t per_xcd = std::max(1, s.kf_slots / 8);
    return per_xcd - (per_xcd > 8 ? UGT_KF_XCD_MARGIN : 0);
}

/* workgroups per lane for n lanes: the lanes' clusters share the XCDs evenly (lane z on XCD z % 8) and must all be resident */
static inline int32_t
ug_kf_choose_c(const UgShape &s, const UgEngine &e, int32_t alone, int32_t n)
{
    using std::max; using std::min;
    const int32_t usable = ug_kf_usable(s), per_xcd = max(1, s.kf_slots / 8), lanes_per_xcd = max(1, ug_ceil(n, 8));
    int32_t C = 1;
    if (s.cluster > 0) C = s.cluster;
    else if (alone) {
        const int32_t cmax = e.big_wl ? UGT_KF_CLUSTER_MAX_WIDE : ug_kf_cluster_max(n);
        C = min(per_xcd / lanes_per_xcd, cmax);
        /* ... but an EVEN fill first: a cluster is as fast as its slowest workgroup, and with one and a half workgroups per CU some share
         * a CU and some do not -- 128 lanes: 429.5 k frames/s as clusters of 2 (one workgroup per CU) against 406.9 k as clusters of 3
         * (profiles/r6_experiments.txt 16).  So: as many workgroups per lane as still leave every workgroup a CU of its own, when that is
         * a cluster at all */
        const int32_t c1 = min(max(1, s.n_cu / 8) / lanes_per_xcd, cmax);
        if (c1 >= 2) C = c1;
    }
    /* (KF_MAXC: what the kernel's LDS arrays -- the waves' segments, the cluster's scan -- are sized for) */
    return max(1, min(min(C, (int32_t)UGC_KF_MAXC), usable / lanes_per_xcd));
}

static inline int32_t ug_kf_grid(int32_t C, int32_t n) { return C == 1 ? n : 8 * C * ug_ceil(n, 8); }

/* the lead and the rounds handed to kf_plan for `first` lanes scored beside the search: the lead in groups of 8 frames (kf_overlap_lead, or
 * UGC_KF_LEAD frames), a round as many groups of each first utterance as make one scoring launch of UGC_PIECE groups (kf_overlap_round) */
static inline void
ug_kf_rounds(const UgCall &c, int32_t first, int32_t *lead_g, int32_t *round_g)
{
    const int32_t lg = ug_ceil(std::max(0, c.kf_overlap_lead), UGC_UW_FB);
    *lead_g = lg > 0 ? lg : UGC_KF_LEAD / UGC_UW_FB;
    *round_g = c.kf_overlap_round > 0 ? c.kf_overlap_round : std::max(1, UGC_PIECE / std::max(1, first));
}

/* a ku_frames call over n lane slots.  ov: its first launch is the three of scoring beside the search (one workgroup per lane).
 * THE RELAY: when nothing is left to take and no more lanes are at work than fit the chip as clusters of 2 (then 4) workgroups, they hand
 * themselves over to the chain's next launch: stage k runs at most st_cap lanes as clusters of st_c, and only when that is fewer lanes than
 * 0.8 of the launch before.  Only an engine that may size clusters for the whole device plans a chain (not with .cluster set: the caller's
 * cluster size holds for the whole call); kf_relay_at, the tests' switch: the chain from one workgroup per lane on, however few the lanes and
 * whatever else runs on the device; kf_no_relay: never.
 * n1: SCORING BESIDE THE SEARCH, only where its premise holds -- an engine that sizes its launches for the whole device, two lanes per CU
 * (more lanes than CUs, half of them no more), one workgroup per lane, more utterances than lanes -- and only for the plain call: no second
 * pass, no look-ahead heuristic, no kept lattices, no .cluster.  kf_overlap_n1 > 0 forces it with that many first lanes (< lanes; the call's
 * own conditions still hold), kf_no_overlap: never.  (The plan drops n1 again when the queue goes through in more than one part.) */
static inline UgKf
ug_kf(const UgShape &s, const UgEngine &e, const UgCall &c, int32_t n, int32_t ov)
{
    using std::max; using std::min;
    UgKf k = {};
    k.served = ug_kf_served(s, e, c, n);
    k.usable = ug_kf_usable(s);
    k.C = ug_kf_choose_c(s, e, c.alone, n);
    k.grid = ug_kf_grid(k.C, n);
    k.c0 = (c.kf_relay_at > 0 && s.cluster == 0) || ov ? 1 : k.C;
    k.grid0 = ug_kf_grid(k.c0, n);
    if (s.cluster == 0 && (c.alone || c.kf_relay_at > 0) && !c.kf_no_relay) {
        int32_t prev_n = n, prev_c = k.c0, st[UGC_KF_STAGES][3] = {};
        for (int32_t cc = 2; cc <= 4 && k.n_st < UGC_KF_STAGES; cc *= 2) {
            int32_t cap = 8 * (k.usable / cc);
            if (c.kf_relay_at > 0) cap = min(cap, max(1, c.kf_relay_at / (cc / 2)));
            /* (fewer lanes than 0.8 of the launch before; and at least one: an XCD that holds fewer than cc workgroups has no such stage) */
            if (cc <= prev_c || cap < 1 || (int64_t)cap * 5 > (int64_t)prev_n * 4) continue;
            st[k.n_st][0] = cc; st[k.n_st][1] = cap; st[k.n_st][2] = ug_kf_grid(cc, cap);
            k.n_st++;
            prev_n = cap; prev_c = cc;
        }
        k.st_c1 = st[0][0]; k.st_cap1 = st[0][1]; k.st_grid1 = st[0][2];
        k.st_c2 = st[1][0]; k.st_cap2 = st[1][1]; k.st_grid2 = st[1][2];
    }
    if (c.queue && !c.kf_no_overlap && !c.second_pass && s.pheurtype == 0 && !c.keep_lat && c.n_utt > s.n_lanes && s.cluster == 0) {
        const int32_t n_cu = max(1, s.n_cu);
        if (c.kf_overlap_n1 > 0) { if (c.kf_overlap_n1 < s.n_lanes) k.n1 = c.kf_overlap_n1; }
        else if (c.alone && s.n_lanes > n_cu && s.n_lanes / 2 <= n_cu && ug_kf_choose_c(s, e, c.alone, s.n_lanes) == 1) k.n1 = s.n_lanes / 2;
    }
    ug_kf_rounds(c, k.n1, &k.lead_g, &k.round_g);
    return k;
}

/* ---- what a call runs as.  max_rows: the rows of senone scores the largest part of the call's plan needs; budget: what the device holds ---- */
static inline int32_t
ug_route(const UgShape &s, const UgEngine &e, const UgCall &c, int64_t max_rows, int64_t budget)
{
    const int32_t n = c.queue ? std::min(s.n_lanes, c.n_utt) : c.n_utt;
    if (e.use_graph && c.prof_every == 0) return UG_ROUTE_GRAPH;
    const bool served = ug_kf_served(s, e, c, n), fits = max_rows <= budget;
    if (!c.queue) return !served ? UG_ROUTE_FRAMES : fits ? UG_ROUTE_KF_STATIC : UG_ROUTE_WINDOW;
    if (!served) return UG_ROUTE_FRAMES;
    /* (the plain queue is KF_QUEUE whatever its size: it goes through in parts.  With the second pass or -pheurtype: groups of static
     * launches -- the look-ahead's tables are a LANE's --, and where a group's scores do not fit, window blocks only when asked for:
     * they keep all lanes in step, the regime that lost to the launches) */
    if (!c.second_pass && s.pheurtype == 0) return UG_ROUTE_KF_QUEUE;
    return fits ? UG_ROUTE_KF_GROUPS : e.persist > 1 ? UG_ROUTE_WINDOW : UG_ROUTE_FRAMES;
}
#endif
