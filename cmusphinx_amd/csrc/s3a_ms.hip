/*
 * s3a_ms.hip -- device half of the multi-stream senone scorer (-senmgau .s3cont. / .semi.).
 *
 * Reference: ms_cont_mgau_frame_eval (sphinx3 libam/ms_mgau.c:242-329) = flag the codebooks of
 * the active senones, gauden_dist (ms_gauden.c:541-644) for each, senone_eval
 * (ms_senone.c:442-490) for each active senone, best, normalise.
 *
 * Layout: codebook parameters are TRANSPOSED per (codebook, stream) to [dim][P] with
 * P = n_density rounded up to a power of two, so that the P lanes that evaluate one
 * codebook read consecutive floats for every dimension (a 32-byte sector per 8-density
 * continuous codebook); the frame's feature vector sits in LDS.
 *
 *   k_ms_mark     codebook flags from the senone mask (skipped when the mapping is 1-to-1)
 *   k_ms_dist     lane = (codebook, stream, density): float64 distance chain in dimension
 *                 order (no FMA), then the ordered top-N list -- the reference's insertion
 *                 sort keeps (distance, codeword) order, i.e. each density's slot is its
 *                 RANK, computed by every lane against its codebook's values in LDS --
 *                 floor, logmath_ln_to_log truncation
 *   k_ms_senone   thread = active senone: per stream the ordered log-add of dist - pdf,
 *                 summed over streams; block max -> atomicMax
 *   k_ms_norm     senscr -= best for the active senones
 *
 * Many frames in one pass (s3a_ms_mgau_score_frames*, at the end of this file): a lane keeps the
 * distances of its density to a TILE of frames in registers while the dimensions stream past, so
 * the parameters are read once per tile, not once per frame; the tile's features sit in LDS as
 * [dim][frame].  Two shapes, chosen by the model:
 *
 *   k_msb_cont    ".s3cont." (codebook s <=> senone s): distances, ranks through LDS, and the
 *                 senone's ordered log-add in place -- the top-N lists never reach memory
 *   k_msb_topn    shared codebooks: the top-N lists of (frame, codebook, stream) into scratch, then
 *   k_msb_senone  thread = (frame, senone): gathers pdf[s][f][id[t]], ordered log-add, frame max
 *   k_msb_norm    rows -= best for the active entries (not with S3A_MS_RAW)
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <vector>

#include "s3a_device.h"

#define MSB 256

struct s3a_ms_dev_s {
    int32_t P;                      /* padded densities per codebook-stream */
    float *meanT, *precT;           /* per (m, f): [featlen f][P], blocks in (m, f) order */
    float *det;                     /* [m][f][P] */
    int32_t *featlen, *featoff;     /* device copies */
    int32_t *pdf, *mgau;
    uint32_t *tab;                  /* log-add table widened to u32 */
    uint32_t tab_size;
    int32_t lm_zero;
    uint8_t *sen_active, *mgau_active;
    float *feat;
    int32_t *dist, *dist_id, *scr, *best;
    int32_t *scr_h, *best_h;        /* pinned */
    hipStream_t stream;
    /* block scoring (s3a_ms_mgau_score_frames*): scratch that grows on demand */
    int32_t blk_ft;                 /* frames per tile: 16, 4 or 1, by the feature vector's length */
    int32_t blk_chunk;              /* s3a_ms_mgau_set_block_chunk: 0 = the library's choice */
    s3a_grow<int2> blk_lists;       /* shared codebooks: [frame][m][f][topn] (distance, codeword) */
    s3a_grow<int32_t> blk_best;     /* [frame] for a caller that wants no best */
    s3a_grow<float> blk_feat;       /* the host variant's staging: features, masks, rows, best */
    s3a_grow<uint8_t> blk_act;
    s3a_grow<int32_t> blk_scr, blk_bst;     /* device + pinned */
    s3a_hostmem mem;                /* every device / pinned buffer above is its */
};

struct LogAdd32 {
    const uint32_t *tab;
    uint32_t size;
    int32_t zero;
    __device__ __forceinline__ int32_t operator()(int32_t x, int32_t y) const
    {
        if (x <= zero) return y;
        if (y <= zero) return x;
        const int32_t hi = x > y ? x : y, lo = x > y ? y : x;
        const uint32_t d = (uint32_t)hi - (uint32_t)lo;
        if (d >= size) return hi;
        return hi + (int32_t)tab[d];
    }
};

__global__ void
k_ms_mark(const uint8_t *__restrict__ sen_active, const int32_t *__restrict__ mgau, int32_t n_sen,
          uint8_t *mgau_active)
{
    const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_sen && sen_active[s]) mgau_active[mgau[s]] = 1;
}

__global__ void __launch_bounds__(MSB)
k_ms_dist(int32_t n_mgau, int32_t n_feat, int32_t nd, int32_t P, int32_t veclen, int32_t topn,
          const int32_t *__restrict__ featlen, const int32_t *__restrict__ featoff,
          const float *__restrict__ meanT, const float *__restrict__ precT, const float *__restrict__ det,
          const uint8_t *__restrict__ mgau_active, const float *__restrict__ feat, double min_density,
          double inv_log_of_base, int32_t shift, int32_t *dist, int32_t *dist_id)
{
    extern __shared__ float x_s[];              /* [veclen] */
    __shared__ double dv[MSB];
    for (int32_t i = threadIdx.x; i < veclen; i += MSB) x_s[i] = feat[i];
    __syncthreads();
    const int32_t item = blockIdx.x * MSB + threadIdx.x;
    const int32_t job = item / P, d = item % P;             /* job = m * n_feat + f */
    const int32_t m = job / n_feat, f = job % n_feat;
    const bool live = job < n_mgau * n_feat && mgau_active[m] != 0;
    double dval = 0.0;
    if (live && d < nd) {
        const int32_t flen = featlen[f], fo = featoff[f];
        const size_t base = ((size_t)m * veclen + fo) * P;      /* start of the (m, f) block */
        dval = (double)det[(size_t)job * P + d];
        for (int32_t i = 0; i < flen; i++) {
            const float df = x_s[fo + i] - meanT[base + (size_t)i * P + d];     /* float32 subtract */
            const double dd = (double)df;
            const double t = (dd * dd) * (double)precT[base + (size_t)i * P + d];
            dval = dval + t;                                                    /* not an fma */
        }
    }
    dv[threadIdx.x] = dval;
    __syncthreads();
    if (!live || d >= nd) return;
    int32_t rank = d;
    if (topn < nd) {
        /* slot in the reference's ordered list: densities with a smaller distance, or an equal
         * one and a smaller codeword id, come first */
        const double *mine = dv + (threadIdx.x - d);
        rank = 0;
        for (int32_t k = 0; k < nd; k++) {
            const double o = mine[k];
            rank += (o < dval || (o == dval && k < d)) ? 1 : 0;
        }
        if (rank >= topn) return;
    }
    double v = -dval;
    if (v < min_density) v = min_density;
    const size_t o = (size_t)job * topn + rank;
    dist_id[o] = d;
    dist[o] = (int32_t)(v * inv_log_of_base) >> shift;
}

__global__ void __launch_bounds__(MSB)
k_ms_senone(int32_t n_sen, int32_t n_feat, int32_t nd, int32_t topn, const uint8_t *__restrict__ sen_active,
            const int32_t *__restrict__ mgau, const int32_t *__restrict__ pdf, const int32_t *__restrict__ dist,
            const int32_t *__restrict__ dist_id, LogAdd32 la, int32_t *scr, int32_t *best)
{
    __shared__ int32_t red[MSB / 64];
    const int32_t s = blockIdx.x * MSB + threadIdx.x;
    int32_t v = INT_MIN;
    if (s < n_sen && sen_active[s]) {
        const int32_t m = mgau[s];
        uint32_t tot = 0;
        for (int32_t f = 0; f < n_feat; f++) {
            const int32_t *fd = dist + ((size_t)m * n_feat + f) * topn, *fi = dist_id + ((size_t)m * n_feat + f) * topn;
            const int32_t *p = pdf + ((size_t)s * n_feat + f) * nd;
            int32_t fscr = (int32_t)((uint32_t)fd[0] - (uint32_t)p[fi[0]]);
            for (int32_t t = 1; t < topn; t++)
                fscr = la(fscr, (int32_t)((uint32_t)fd[t] - (uint32_t)p[fi[t]]));
            tot += (uint32_t)fscr;
        }
        v = (int32_t)tot;
        scr[s] = v;
    }
    int32_t b = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b = max(b, __shfl_xor(b, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MSB / 64; w++) b = max(b, red[w]);
        if (b != INT_MIN) atomicMax(best, b);
    }
}

__global__ void
k_ms_norm(int32_t n_sen, const uint8_t *__restrict__ sen_active, const int32_t *__restrict__ best, int32_t *scr)
{
    const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_sen && sen_active[s]) scr[s] = (int32_t)((uint32_t)scr[s] - (uint32_t)*best);
}

/* ------------------------------------------------------------------ */
#define DM(ptr, bytes) do { if (!dv->mem.dev(ptr, bytes)) return S3A_EHIP; } while (0)

/* (a failure leaves what was made so far to s3a_ms_dev_create, which destroys it) */
static int32_t
ms_dev_fill(s3a_ms_mgau_t *ms)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        s3a_set_error("no HIP device: libcmusphinx_amd has no CPU fallback");
        return S3A_ENODEV;
    }
    int32_t P = 1;
    while (P < ms->n_density) P <<= 1;
    if (P > MSB) {
        s3a_set_error("s3a_ms_mgau_init: %d densities per codebook exceed the kernel's %d", ms->n_density, MSB);
        return S3A_EUNSUP;
    }
    if (ms->veclen * 4 > 48 * 1024) { s3a_set_error("s3a_ms_mgau_init: feature vector too long"); return S3A_EUNSUP; }
    s3a_ms_dev_s *dv = new s3a_ms_dev_s();     /* (value-initialised) */
    ms->dev = dv;
    dv->P = P;
    dv->blk_ft = ms->veclen * 4 * 16 <= 48 * 1024 ? 16 : ms->veclen * 4 * 4 <= 48 * 1024 ? 4 : 1;
    const int32_t M = ms->n_mgau, F = ms->n_feat, nd = ms->n_density, D = ms->veclen, S = ms->n_sen;
    const size_t nT = (size_t)M * D * P;
    std::vector<float> mt(nT, 0.0f), pt(nT, 0.0f), dt((size_t)M * F * P, 0.0f);
    for (int32_t m = 0; m < M; m++)
        for (int32_t f = 0; f < F; f++) {
            const size_t src = (size_t)m * nd * D + (size_t)nd * ms->featoff[f];
            const size_t dst = ((size_t)m * D + ms->featoff[f]) * P;
            for (int32_t d = 0; d < nd; d++) {
                dt[((size_t)m * F + f) * P + d] = ms->det[((size_t)m * F + f) * nd + d];
                for (int32_t i = 0; i < ms->featlen[f]; i++) {
                    mt[dst + (size_t)i * P + d] = ms->mean[src + (size_t)d * ms->featlen[f] + i];
                    pt[dst + (size_t)i * P + d] = ms->prec[src + (size_t)d * ms->featlen[f] + i];
                }
            }
        }
    HIPCHK(hipStreamCreateWithFlags(&dv->stream, hipStreamNonBlocking));
    DM(dv->meanT, nT * 4); DM(dv->precT, nT * 4); DM(dv->det, (size_t)M * F * P * 4);
    DM(dv->featlen, (size_t)F * 4); DM(dv->featoff, (size_t)(F + 1) * 4);
    DM(dv->pdf, (size_t)S * F * nd * 4); DM(dv->mgau, (size_t)S * 4);
    DM(dv->sen_active, (size_t)S); DM(dv->mgau_active, (size_t)M); DM(dv->feat, (size_t)D * 4);
    DM(dv->dist, (size_t)M * F * ms->topn * 4); DM(dv->dist_id, (size_t)M * F * ms->topn * 4);
    DM(dv->scr, (size_t)S * 4); DM(dv->best, 4);
    if (!dv->mem.pin(dv->scr_h, (size_t)S * 4) || !dv->mem.pin(dv->best_h, 4)) return S3A_EHIP;
    HIPCHK(hipMemcpy(dv->meanT, mt.data(), nT * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dv->precT, pt.data(), nT * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dv->det, dt.data(), dt.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dv->featlen, ms->featlen, (size_t)F * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dv->featoff, ms->featoff, (size_t)(F + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dv->pdf, ms->pdf, (size_t)S * F * nd * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dv->mgau, ms->mgau, (size_t)S * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dv->dist, 0, (size_t)M * F * ms->topn * 4));
    HIPCHK(hipMemset(dv->dist_id, 0, (size_t)M * F * ms->topn * 4));
    {
        uint32_t size = 0, width = 0, shift = 0;
        s3a_logmath_get_table_shape(ms->lm, &size, &width, &shift);
        dv->tab_size = size;
        dv->lm_zero = s3a_logmath_get_zero(ms->lm);
        if (size == 0) { s3a_set_error("s3a_ms_mgau_init: a logmath without an add table is not supported"); return S3A_EUNSUP; }
        std::vector<uint32_t> tab(size);
        s3a_logmath_copy_table(ms->lm, tab.data(), size);
        DM(dv->tab, (size_t)size * 4);
        HIPCHK(hipMemcpy(dv->tab, tab.data(), (size_t)size * 4, hipMemcpyHostToDevice));
    }
    return S3A_OK;
}

extern "C" int32_t
s3a_ms_dev_create(s3a_ms_mgau_t *ms)
{
    const int32_t rc = ms_dev_fill(ms);
    if (rc != S3A_OK) s3a_ms_dev_destroy(ms);
    return rc;
}

extern "C" void
s3a_ms_dev_destroy(s3a_ms_mgau_t *ms)
{
    s3a_ms_dev_s *dv = ms ? ms->dev : NULL;
    if (!dv) return;
    dv->mem.free_all();
    if (dv->stream) (void)hipStreamDestroy(dv->stream);
    delete dv;
    ms->dev = NULL;
}

extern "C" int32_t
s3a_ms_cont_mgau_frame_eval(s3a_ms_mgau_t *ms, const uint8_t *sen_active, int32_t *senscr, const float *feat,
                            int32_t frame, int32_t *best)
{
    (void)frame;
    if (!ms || !ms->dev || !sen_active || !senscr || !feat || !best) return S3A_EINVAL;
    s3a_ms_dev_s *dv = ms->dev;
    const int32_t M = ms->n_mgau, F = ms->n_feat, nd = ms->n_density, S = ms->n_sen, P = dv->P;
    const int32_t init = INT_MIN;
    HIPCHK(hipMemcpyAsync(dv->sen_active, sen_active, (size_t)S, hipMemcpyHostToDevice, dv->stream));
    HIPCHK(hipMemcpyAsync(dv->feat, feat, (size_t)ms->veclen * 4, hipMemcpyHostToDevice, dv->stream));
    HIPCHK(hipMemcpyAsync(dv->best, &init, 4, hipMemcpyHostToDevice, dv->stream));
    const uint8_t *cb_active = dv->sen_active;             /* ".s3cont.": codebook s <=> senone s */
    if (!ms->one_to_one) {
        HIPCHK(hipMemsetAsync(dv->mgau_active, 0, (size_t)M, dv->stream));
        hipLaunchKernelGGL(k_ms_mark, dim3((S + 255) / 256), dim3(256), 0, dv->stream, dv->sen_active, dv->mgau, S,
                           dv->mgau_active);
        cb_active = dv->mgau_active;
    }
    const int64_t items = (int64_t)M * F * P;
    hipLaunchKernelGGL(k_ms_dist, dim3((uint32_t)((items + MSB - 1) / MSB)), dim3(MSB), (size_t)ms->veclen * 4,
                       dv->stream, M, F, nd, P, ms->veclen, ms->topn, dv->featlen, dv->featoff, dv->meanT,
                       dv->precT, dv->det, cb_active, dv->feat, ms->min_density, ms->lm->inv_log_of_base,
                       ms->lm->shift, dv->dist, dv->dist_id);
    LogAdd32 la = { dv->tab, dv->tab_size, dv->lm_zero };
    hipLaunchKernelGGL(k_ms_senone, dim3((S + MSB - 1) / MSB), dim3(MSB), 0, dv->stream, S, F, nd, ms->topn,
                       dv->sen_active, dv->mgau, dv->pdf, dv->dist, dv->dist_id, la, dv->scr, dv->best);
    hipLaunchKernelGGL(k_ms_norm, dim3((S + 255) / 256), dim3(256), 0, dv->stream, S, dv->sen_active, dv->best,
                       dv->scr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dv->scr_h, dv->scr, (size_t)S * 4, hipMemcpyDeviceToHost, dv->stream));
    HIPCHK(hipMemcpyAsync(dv->best_h, dv->best, 4, hipMemcpyDeviceToHost, dv->stream));
    HIPCHK(hipStreamSynchronize(dv->stream));
    for (int32_t s = 0; s < S; s++)
        if (sen_active[s]) senscr[s] = dv->scr_h[s];
    *best = *dv->best_h;
    return S3A_OK;
}

extern "C" int32_t
s3a_ms_mgau_get_dist(s3a_ms_mgau_t *ms, int32_t *dist, int32_t *dist_id)
{
    if (!ms || !ms->dev || !dist || !dist_id) return S3A_EINVAL;
    const size_t n = (size_t)ms->n_mgau * ms->n_feat * ms->topn * 4;
    HIPCHK(hipStreamSynchronize(ms->dev->stream));
    HIPCHK(hipMemcpy(dist, ms->dev->dist, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dist_id, ms->dev->dist_id, n, hipMemcpyDeviceToHost));
    return S3A_OK;
}

/* ------------------------------------------------------------------ */
/* many frames in one pass                                             */
/* ------------------------------------------------------------------ */
struct MsbArgs {
    int32_t n_mgau, n_feat, nd, P, veclen, topn, n_sen;
    const int32_t *featlen, *featoff;
    const float *meanT, *precT, *det;
    const int32_t *pdf;
    double min_density, inv_log_of_base;
    int32_t shift;
    const float *feat;              /* the part's first frame */
    int32_t feat_stride, n_frames;
};

/* the tile's features into LDS as [dim][FT]; frames behind the last one are zeros (scored, never written) */
template <int FT>
__device__ __forceinline__ void
msb_stage(float *xs, const MsbArgs &A, int32_t f0, int32_t nf)
{
    for (int32_t idx = threadIdx.x; idx < A.veclen * FT; idx += MSB) {
        const int32_t j = idx / A.veclen, i = idx - j * A.veclen;
        xs[i * FT + j] = j < nf ? A.feat[(size_t)(f0 + j) * A.feat_stride + i] : 0.0f;
    }
}

/* gauden_dist's chain for one density and FT frames: the dimensions in order, each parameter read once.
 * xs = the stream's first dimension in LDS; mT / pT = this density's column of the (m, f) block */
template <int FT>
__device__ __forceinline__ void
msb_dist(double (&a)[FT], const float *xs, const float *__restrict__ mT, const float *__restrict__ pT, int32_t P,
         int32_t flen, float det)
{
#pragma unroll
    for (int j = 0; j < FT; j++) a[j] = (double)det;
    float m = mT[0], p = pT[0];
    for (int32_t i = 0; i < flen; i++) {
        const float mc = m;
        const double pc = (double)p;
        if (i + 1 < flen) { m = mT[(size_t)(i + 1) * P]; p = pT[(size_t)(i + 1) * P]; }     /* the next one, under this one's arithmetic */
        float x[FT];
        if constexpr (FT % 4 == 0) {
            const float4 *x4 = (const float4 *)xs + (size_t)i * (FT / 4);      /* every lane the same address: a broadcast */
#pragma unroll
            for (int q = 0; q < FT / 4; q++) {
                const float4 v = x4[q];
                x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
            }
        }
        else {
#pragma unroll
            for (int j = 0; j < FT; j++) x[j] = xs[(size_t)i * FT + j];
        }
#pragma unroll
        for (int j = 0; j < FT; j++) {
            const float df = x[j] - mc;                     /* float32 subtract */
            const double dd = (double)df;
            const double t = (dd * dd) * pc;
            a[j] = a[j] + t;                                /* not an fma */
        }
    }
}

/* slot of density d in the reference's ordered list (as in k_ms_dist); col = the codebook's distances of one frame */
__device__ __forceinline__ int32_t
msb_rank(const double *col, double dval, int32_t d, int32_t nd, int32_t topn)
{
    if (topn >= nd) return d;
    int32_t rank = 0;
    for (int32_t k = 0; k < nd; k++) {
        const double o = col[k];
        rank += (o < dval || (o == dval && k < d)) ? 1 : 0;
    }
    return rank;
}

__device__ __forceinline__ int32_t
msb_to_int(double dval, const MsbArgs &A)
{
    double v = -dval;
    if (v < A.min_density) v = A.min_density;
    return (int32_t)(v * A.inv_log_of_base) >> A.shift;
}

/* LDS of the two tile kernels: [distances FT x MSB f64][features veclen x FT f32, padded to 16 bytes] and, for
 * k_msb_cont, [dist - pdf in list order: FT x codebooks x topn][stream sums: FT x codebooks][frame max: FT] */
static size_t
msb_lds_bytes(int32_t ft, int32_t veclen, int32_t P, int32_t topn, bool cont)
{
    size_t b = (size_t)ft * MSB * 8 + ((((size_t)veclen * ft + 3) & ~(size_t)3) * 4);
    if (cont) b += ((size_t)ft * (MSB / P) * topn + (size_t)ft * (MSB / P) + ft) * 4;
    return b;
}

/* ".s3cont.": grid (codebooks / (MSB / P), frame tiles); lane = (codebook = senone, density) */
template <int FT>
__global__ void __launch_bounds__(MSB)
k_msb_cont(MsbArgs A, LogAdd32 la, const uint8_t *__restrict__ act, int32_t *senscr, int32_t row_stride, int32_t *best)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char msb_smem[];
    const int32_t tid = threadIdx.x, P = A.P, CB = MSB / P, topn = A.topn;
    double *dvs = (double *)msb_smem;
    float *xs = (float *)(dvs + FT * MSB);
    int32_t *vals = (int32_t *)(xs + (((size_t)A.veclen * FT + 3) & ~(size_t)3));
    uint32_t *tot = (uint32_t *)(vals + FT * CB * topn);
    int32_t *bestj = (int32_t *)(tot + FT * CB);
    const int32_t f0 = blockIdx.y * FT, nf = min(FT, A.n_frames - f0);
    const int32_t jl = tid / P, d = tid - jl * P, cb0 = blockIdx.x * CB, cb = cb0 + jl;
    const bool live = cb < A.n_sen && d < A.nd;

    msb_stage<FT>(xs, A, f0, nf);
    if (tid < FT) bestj[tid] = INT_MIN;
    __syncthreads();
    for (int32_t f = 0; f < A.n_feat; f++) {
        double a[FT];
        if (live) {
            const int32_t fo = A.featoff[f];
            const size_t base = ((size_t)cb * A.veclen + fo) * P + d;
            msb_dist<FT>(a, xs + (size_t)fo * FT, A.meanT + base, A.precT + base, P, A.featlen[f],
                         A.det[((size_t)cb * A.n_feat + f) * P + d]);
        }
        else {
#pragma unroll
            for (int j = 0; j < FT; j++) a[j] = 0.0;
        }
#pragma unroll
        for (int j = 0; j < FT; j++) dvs[j * MSB + tid] = a[j];
        __syncthreads();
        if (live) {
            /* a senone's own codebook: the weight goes in here, and the list holds dist - pdf */
            const uint32_t w = (uint32_t)A.pdf[((size_t)cb * A.n_feat + f) * A.nd + d];
            for (int32_t j = 0; j < nf; j++) {
                const double *col = dvs + j * MSB + (tid - d);
                const double dval = col[d];
                const int32_t rank = msb_rank(col, dval, d, A.nd, topn);
                if (rank < topn) vals[(j * CB + jl) * topn + rank] = (int32_t)((uint32_t)msb_to_int(dval, A) - w);
            }
        }
        __syncthreads();
        /* the ordered log-add, one thread per (frame, senone); an item stays with its thread over the streams */
        for (int32_t item = tid; item < FT * CB; item += MSB) {
            const int32_t j = item / CB, c = item - j * CB;
            if (j >= nf || cb0 + c >= A.n_sen) continue;
            const int32_t *v = vals + item * topn;
            int32_t fscr = v[0];
            for (int32_t t = 1; t < topn; t++) fscr = la(fscr, v[t]);
            tot[item] = f == 0 ? (uint32_t)fscr : tot[item] + (uint32_t)fscr;
        }
        /* (the next stream writes vals only behind its first barrier, which every thread reaches after this loop) */
    }
    for (int32_t item = tid; item < FT * CB; item += MSB) {
        const int32_t j = item / CB, c = item - j * CB, s = cb0 + c;
        if (j >= nf || s >= A.n_sen) continue;
        if (act && !act[(size_t)(f0 + j) * A.n_sen + s]) continue;
        const int32_t v = (int32_t)tot[item];
        senscr[(size_t)(f0 + j) * row_stride + s] = v;
        atomicMax(&bestj[j], v);
    }
    __syncthreads();
    if (tid < nf && bestj[tid] != INT_MIN) atomicMax(best + f0 + tid, bestj[tid]);
}

/* shared codebooks, phase 1: grid ((codebook, stream) jobs / (MSB / P), frame tiles); lists [frame][job][topn] */
template <int FT>
__global__ void __launch_bounds__(MSB)
k_msb_topn(MsbArgs A, int2 *__restrict__ lists)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char msb_smem[];
    const int32_t tid = threadIdx.x, P = A.P, CB = MSB / P, topn = A.topn, jobs = A.n_mgau * A.n_feat;
    double *dvs = (double *)msb_smem;
    float *xs = (float *)(dvs + FT * MSB);
    const int32_t f0 = blockIdx.y * FT, nf = min(FT, A.n_frames - f0);
    const int32_t jl = tid / P, d = tid - jl * P, job = blockIdx.x * CB + jl;
    const bool live = job < jobs && d < A.nd;

    msb_stage<FT>(xs, A, f0, nf);
    __syncthreads();
    double a[FT];
    if (live) {
        const int32_t m = job / A.n_feat, f = job - m * A.n_feat, fo = A.featoff[f];
        const size_t base = ((size_t)m * A.veclen + fo) * P + d;
        msb_dist<FT>(a, xs + (size_t)fo * FT, A.meanT + base, A.precT + base, P, A.featlen[f], A.det[(size_t)job * P + d]);
    }
    else {
#pragma unroll
        for (int j = 0; j < FT; j++) a[j] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < FT; j++) dvs[j * MSB + tid] = a[j];
    __syncthreads();
    if (!live) return;
    for (int32_t j = 0; j < nf; j++) {
        const double *col = dvs + j * MSB + (tid - d);
        const double dval = col[d];
        const int32_t rank = msb_rank(col, dval, d, A.nd, topn);
        if (rank < topn) lists[((size_t)(f0 + j) * jobs + job) * topn + rank] = make_int2(msb_to_int(dval, A), d);
    }
}

/* shared codebooks, phase 2: grid (senones / MSB, frames); k_ms_senone with a frame's lists and rows */
__global__ void __launch_bounds__(MSB)
k_msb_senone(int32_t n_sen, int32_t n_feat, int32_t nd, int32_t topn, int32_t jobs, const uint8_t *__restrict__ act,
             const int32_t *__restrict__ mgau, const int32_t *__restrict__ pdf, const int2 *__restrict__ lists, LogAdd32 la,
             int32_t *senscr, int32_t row_stride, int32_t *best)
{
    __shared__ int32_t red[MSB / 64];
    const int32_t s = blockIdx.x * MSB + threadIdx.x, fr = blockIdx.y;
    int32_t v = INT_MIN;
    if (s < n_sen && (!act || act[(size_t)fr * n_sen + s])) {
        const int32_t m = mgau[s];
        uint32_t tot = 0;
        for (int32_t f = 0; f < n_feat; f++) {
            const int2 *l = lists + ((size_t)fr * jobs + (size_t)m * n_feat + f) * topn;
            const int32_t *p = pdf + ((size_t)s * n_feat + f) * nd;
            int32_t fscr = (int32_t)((uint32_t)l[0].x - (uint32_t)p[l[0].y]);
            for (int32_t t = 1; t < topn; t++)
                fscr = la(fscr, (int32_t)((uint32_t)l[t].x - (uint32_t)p[l[t].y]));
            tot += (uint32_t)fscr;
        }
        v = (int32_t)tot;
        senscr[(size_t)fr * row_stride + s] = v;
    }
    int32_t b = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b = max(b, __shfl_xor(b, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MSB / 64; w++) b = max(b, red[w]);
        if (b != INT_MIN) atomicMax(best + fr, b);
    }
}

__global__ void __launch_bounds__(MSB)
k_msb_norm(int32_t n_sen, const uint8_t *__restrict__ act, const int32_t *__restrict__ best, int32_t *senscr,
           int32_t row_stride)
{
    const int32_t s = blockIdx.x * MSB + threadIdx.x, fr = blockIdx.y;
    if (s < n_sen && (!act || act[(size_t)fr * n_sen + s])) {
        int32_t *p = senscr + (size_t)fr * row_stride + s;
        *p = (int32_t)((uint32_t)*p - (uint32_t)best[fr]);
    }
}

#define MSB_CHUNK_MAX 32768         /* frames per pass: a grid's y extent */

/* frames per internal pass: the hook's, or what keeps the top-N scratch of shared codebooks within 64 MB */
static int32_t
msb_chunk(const s3a_ms_mgau_t *ms)
{
    if (ms->dev->blk_chunk > 0) return ms->dev->blk_chunk;
    if (ms->one_to_one) return 4096;
    const size_t per_frame = (size_t)ms->n_mgau * ms->n_feat * ms->topn * sizeof(int2);
    const size_t c = ((size_t)64 << 20) / per_frame;
    return c < 1 ? 1 : c > 4096 ? 4096 : (int32_t)c;
}

template <int FT>
static int32_t
msb_launch(s3a_ms_mgau_t *ms, const MsbArgs &A, const uint8_t *act, int32_t *scr, int32_t row_stride, int32_t *best,
           hipStream_t st)
{
    s3a_ms_dev_s *dv = ms->dev;
    const int32_t CB = MSB / dv->P, tiles = (A.n_frames + FT - 1) / FT;
    const size_t lds = msb_lds_bytes(FT, ms->veclen, dv->P, ms->topn, ms->one_to_one != 0);
    LogAdd32 la = { dv->tab, dv->tab_size, dv->lm_zero };
    if (ms->one_to_one) {
        if (lds > 64 * 1024)
            HIPCHK(hipFuncSetAttribute((const void *)k_msb_cont<FT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_msb_cont<FT>, dim3((ms->n_sen + CB - 1) / CB, tiles), dim3(MSB), lds, st, A, la, act, scr,
                           row_stride, best);
    }
    else {
        const int32_t jobs = ms->n_mgau * ms->n_feat;
        if (lds > 64 * 1024)
            HIPCHK(hipFuncSetAttribute((const void *)k_msb_topn<FT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_msb_topn<FT>, dim3((jobs + CB - 1) / CB, tiles), dim3(MSB), lds, st, A, dv->blk_lists.d);
        hipLaunchKernelGGL(k_msb_senone, dim3((ms->n_sen + MSB - 1) / MSB, A.n_frames), dim3(MSB), 0, st, ms->n_sen,
                           ms->n_feat, ms->n_density, ms->topn, jobs, act, dv->mgau, dv->pdf, dv->blk_lists.d, la, scr,
                           row_stride, best);
    }
    HIPCHK(hipGetLastError());
    return S3A_OK;
}

/* one pass: n <= msb_chunk(ms) frames, everything on the device, asynchronous on st */
static int32_t
msb_pass(s3a_ms_mgau_t *ms, const float *feat, int32_t feat_stride, int32_t n, const uint8_t *act, int32_t *scr,
         int32_t row_stride, int32_t *best, int32_t flags, hipStream_t st)
{
    s3a_ms_dev_s *dv = ms->dev;
    if (!best) {
        const int32_t rc = dv->blk_best.reserve(dv->mem, S3A_GROW_DEV, (size_t)n, (size_t)n);
        if (rc != S3A_OK) return rc;
        best = dv->blk_best.d;
    }
    if (!ms->one_to_one) {
        const size_t need = (size_t)n * ms->n_mgau * ms->n_feat * ms->topn;
        if (need > dv->blk_lists.cap) {
            const int32_t rc = dv->blk_lists.reserve(dv->mem, S3A_GROW_DEV, need, need);
            if (rc != S3A_OK) return rc;
            /* (a slot that no density claims -- a NaN distance -- then holds codeword 0, not an index out of the weights) */
            HIPCHK(hipMemsetAsync(dv->blk_lists.d, 0, need * sizeof(int2), st));
        }
    }
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)best, INT_MIN, (size_t)n, st));
    MsbArgs A = { ms->n_mgau, ms->n_feat, ms->n_density, dv->P, ms->veclen, ms->topn, ms->n_sen, dv->featlen, dv->featoff,
                  dv->meanT, dv->precT, dv->det, dv->pdf, ms->min_density, ms->lm->inv_log_of_base, ms->lm->shift,
                  feat, feat_stride, n };
    const int32_t rc = dv->blk_ft == 16 ? msb_launch<16>(ms, A, act, scr, row_stride, best, st)
                     : dv->blk_ft == 4 ? msb_launch<4>(ms, A, act, scr, row_stride, best, st)
                                       : msb_launch<1>(ms, A, act, scr, row_stride, best, st);
    if (rc != S3A_OK) return rc;
    if (!(flags & S3A_MS_RAW)) {
        hipLaunchKernelGGL(k_msb_norm, dim3((ms->n_sen + MSB - 1) / MSB, n), dim3(MSB), 0, st, ms->n_sen, act, best, scr,
                           row_stride);
        HIPCHK(hipGetLastError());
    }
    return S3A_OK;
}

extern "C" int32_t
s3a_ms_mgau_set_block_chunk(s3a_ms_mgau_t *ms, int32_t frames)
{
    if (!ms || !ms->dev || frames < 0) return S3A_EINVAL;
    ms->dev->blk_chunk = frames > MSB_CHUNK_MAX ? MSB_CHUNK_MAX : frames;
    return S3A_OK;
}

extern "C" int32_t
s3a_ms_mgau_score_frames_dev(s3a_ms_mgau_t *ms, const float *feat_dev, int32_t feat_stride, int32_t n_frames,
                             const uint8_t *sen_active_dev, int32_t *senscr_dev, int32_t row_stride, int32_t *best_dev,
                             int32_t flags, void *stream)
{
    if (!ms || !ms->dev || !feat_dev || !senscr_dev || n_frames < 0 || feat_stride < ms->veclen || row_stride < ms->n_sen)
        return S3A_EINVAL;
    hipStream_t st = stream ? (hipStream_t)stream : ms->dev->stream;
    const int32_t chunk = msb_chunk(ms);
    for (int32_t t0 = 0; t0 < n_frames; t0 += chunk) {
        const int32_t n = n_frames - t0 < chunk ? n_frames - t0 : chunk;
        const int32_t rc = msb_pass(ms, feat_dev + (size_t)t0 * feat_stride, feat_stride, n,
                                    sen_active_dev ? sen_active_dev + (size_t)t0 * ms->n_sen : NULL,
                                    senscr_dev + (size_t)t0 * row_stride, row_stride, best_dev ? best_dev + t0 : NULL, flags, st);
        if (rc != S3A_OK) return rc;
    }
    return S3A_OK;
}

extern "C" int32_t
s3a_ms_mgau_score_frames(s3a_ms_mgau_t *ms, const float *feat, int32_t n_frames, const uint8_t *sen_active,
                         int32_t *senscr, int32_t *best, int32_t flags)
{
    if (!ms || !ms->dev || !feat || !senscr || n_frames < 0) return S3A_EINVAL;
    if (n_frames == 0) return S3A_OK;
    s3a_ms_dev_s *dv = ms->dev;
    const size_t S = (size_t)ms->n_sen, D = (size_t)ms->veclen;
    /* a part = one internal pass, and at most 32 MB of rows in the pinned staging */
    size_t part = ((size_t)32 << 20) / (S * 4);
    if (part < 1) part = 1;
    if (part > (size_t)msb_chunk(ms)) part = (size_t)msb_chunk(ms);
    if (part > (size_t)n_frames) part = (size_t)n_frames;
    int32_t rc;
    if ((rc = dv->blk_feat.reserve(dv->mem, S3A_GROW_DEV, part * D, part * D)) != S3A_OK
        || (sen_active && (rc = dv->blk_act.reserve(dv->mem, S3A_GROW_DEV, part * S, part * S)) != S3A_OK)
        || (rc = dv->blk_scr.reserve(dv->mem, S3A_GROW_DEV | S3A_GROW_PIN, part * S, part * S)) != S3A_OK
        || (rc = dv->blk_bst.reserve(dv->mem, S3A_GROW_DEV | S3A_GROW_PIN, part, part)) != S3A_OK)
        return rc;
    for (size_t t0 = 0; t0 < (size_t)n_frames; t0 += part) {
        const size_t n = (size_t)n_frames - t0 < part ? (size_t)n_frames - t0 : part;
        HIPCHK(hipMemcpyAsync(dv->blk_feat.d, feat + t0 * D, n * D * 4, hipMemcpyHostToDevice, dv->stream));
        if (sen_active)
            HIPCHK(hipMemcpyAsync(dv->blk_act.d, sen_active + t0 * S, n * S, hipMemcpyHostToDevice, dv->stream));
        rc = msb_pass(ms, dv->blk_feat.d, (int32_t)D, (int32_t)n, sen_active ? dv->blk_act.d : NULL, dv->blk_scr.d, (int32_t)S,
                      dv->blk_bst.d, flags, dv->stream);
        if (rc != S3A_OK) return rc;
        HIPCHK(hipMemcpyAsync(dv->blk_scr.h, dv->blk_scr.d, n * S * 4, hipMemcpyDeviceToHost, dv->stream));
        HIPCHK(hipMemcpyAsync(dv->blk_bst.h, dv->blk_bst.d, n * 4, hipMemcpyDeviceToHost, dv->stream));
        HIPCHK(hipStreamSynchronize(dv->stream));
        /* only the active entries: the others are the caller's */
        for (size_t t = 0; t < n; t++) {
            int32_t *row = senscr + (t0 + t) * S;
            const int32_t *got = dv->blk_scr.h + t * S;
            if (!sen_active) { memcpy(row, got, S * 4); continue; }
            const uint8_t *a = sen_active + (t0 + t) * S;
            for (size_t s = 0; s < S; s++)
                if (a[s]) row[s] = got[s];
        }
        if (best) memcpy(best + t0, dv->blk_bst.h, n * 4);
    }
    return S3A_OK;
}
