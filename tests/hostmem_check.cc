/*
 * tests/hostmem_check.cc -- TEST INFRASTRUCTURE: cmusphinx_amd/csrc/s3a_hostmem.h on the CPU (tests/test_hostmem.py builds this with the
 * address and undefined-behaviour sanitizers and runs it).  The four allocation functions are malloc-backed stand-ins that count,
 * remember what is live and fail at the k-th allocation; one scripted life of an owner and its growing buffers runs with no failure
 * and with a failure at every allocation of the script in turn.  The life includes a function's stack-local owner left with live
 * buffers on every return path, a buffer taken out of it for the caller (forget), and pinned memory asked for with flags.
 */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <type_traits>
#include "cmusphinx_amd.h"      /* S3A_OK, S3A_ENOMEM */

typedef int hipError_t;
static const hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;

static std::map<void *, int> g_live;    /* pointer -> 1 device, 2 pinned */
static int g_allocs, g_fail_at, g_bad;
static size_t g_last_bytes;
static unsigned g_last_flags;
static char g_err[256];

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "hostmem_check: %s:%d: fail_at %d: %s\n", __FILE__, __LINE__, g_fail_at, #c); g_bad++; } } while (0)

static hipError_t
fake_alloc(void **p, size_t bytes, int kind)
{
    *p = NULL;
    if (++g_allocs == g_fail_at) return hipErrorOutOfMemory;
    CHECK(bytes > 0);
    g_last_bytes = bytes;
    *p = malloc(bytes);
    memset(*p, 0xa5, bytes);
    g_live[*p] = kind;
    return hipSuccess;
}
static hipError_t
fake_free(void *p, int kind)
{
    auto it = g_live.find(p);
    CHECK(it != g_live.end());          /* (never allocated, or freed before) */
    if (it == g_live.end()) return 1;
    CHECK(it->second == kind);          /* (device memory to hipFree, pinned memory to hipHostFree) */
    g_live.erase(it);
    free(p);
    return hipSuccess;
}
static hipError_t hipMalloc(void **p, size_t n) { return fake_alloc(p, n, 1); }
static hipError_t hipHostMalloc(void **p, size_t n, unsigned flags = 0) { g_last_flags = flags; return fake_alloc(p, n, 2); }
static hipError_t hipFree(void *p) { return fake_free(p, 1); }
static hipError_t hipHostFree(void *p) { return fake_free(p, 2); }
static void
s3a_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

#include "s3a_hostmem.h"

/* a function with temporaries of its own: three requests, the second handed to the caller (*out, the caller's to free with hipFree),
 * the others freed by the local owner's scope exit on whichever path it returns */
static bool
temporaries(int32_t **out)
{
    s3a_hostmem tmp;
    int32_t *a = NULL, *keep = NULL;
    float *h = NULL;
    *out = NULL;
    if (!tmp.dev(a, 24) || !tmp.dev(keep, 40)) return false;
    if (!tmp.pin(h, 8, 0x40000000u)) { CHECK(h == NULL); return false; }
    CHECK(g_last_flags == 0x40000000u && g_live[h] == 2 && tmp.recs.size() == 3);
    CHECK(tmp.forget(keep) == false && tmp.recs.size() == 2);       /* (device memory; now nobody's record) */
    CHECK(tmp.forget(keep) == false && tmp.recs.size() == 2);       /* (unknown pointer: nothing) */
    *out = keep;
    return true;
}

/* one life; returns the allocation calls it made */
static int
script(int fail_at)
{
    g_allocs = 0; g_fail_at = fail_at; g_err[0] = 0;
    s3a_hostmem m;
    s3a_grow<int32_t> pair = {}, pinned = {}, dev = {};
    int32_t *a = NULL, *foreign = NULL;
    float *b = NULL;
    const uint8_t *c = NULL;
    void *v = NULL;
    int before;
    /* the owner: mixed kinds, a request of 0 bytes, a const pointer, an early release, a foreign device pointer handed over */
    before = g_allocs;
    if (!m.dev(a, 100)) { CHECK(a == NULL && g_allocs == fail_at && strstr(g_err, "device allocation of 100 bytes failed")); goto done; }
    if (!m.pin(b, 0)) { CHECK(b == NULL && g_allocs == fail_at && strstr(g_err, "pinned allocation of 0 bytes failed")); goto done; }
    CHECK(g_last_bytes == 4);
    if (!m.dev(c, 7)) { CHECK(c == NULL); goto done; }
    if (!m.pin(v, 64)) { CHECK(v == NULL); goto done; }
    CHECK(g_allocs == before + 4 && m.recs.size() == 4 && g_live.size() == 4);
    m.release(b);
    CHECK(b == NULL && m.recs.size() == 3 && g_live.size() == 3);
    m.release(b);                       /* (NULL: nothing) */
    if (hipMalloc((void **)&foreign, 16) == hipSuccess) {
        m.release(foreign);
        CHECK(foreign == NULL && g_live.size() == 3);
    }
    /* a function's local owner: whatever it returns, only what it handed out is still live */
    {
        int32_t *got = NULL;
        const size_t live0 = g_live.size();
        before = g_allocs;
        if (temporaries(&got)) {
            CHECK(got && g_allocs == before + 3 && g_live.size() == live0 + 1 && g_live[got] == 1);
            (void)hipFree(got);
        }
        else CHECK(got == NULL && g_allocs == fail_at);
        CHECK(g_live.size() == live0);
    }
    /* a pair that grows twice, with a reserve that fits in between; a failed reserve leaves it empty and the script goes on */
    for (int round = 0; round < 2; round++) {
        const size_t need = round == 0 ? 10 : 200, grow = need + need / 4 + 64;
        before = g_allocs;
        const int32_t rc = pair.reserve(m, S3A_GROW_DEV | S3A_GROW_PIN, need, grow);
        if (rc != S3A_OK) {
            CHECK(rc == S3A_ENOMEM && pair.d == NULL && pair.h == NULL && pair.cap == 0 && g_live.size() == 3);
            continue;
        }
        CHECK(g_allocs == before + 2 && pair.cap == grow && pair.d && pair.h && g_live[pair.d] == 1 && g_live[pair.h] == 2 && g_live.size() == 5);
        CHECK(g_last_bytes == grow * sizeof(int32_t));
        pair.h[grow - 1] = 1;
        int32_t *d0 = pair.d, *h0 = pair.h;
        before = g_allocs;
        CHECK(pair.reserve(m, S3A_GROW_DEV | S3A_GROW_PIN, need - 1, 1) == S3A_OK && pair.reserve(m, S3A_GROW_DEV | S3A_GROW_PIN, grow, 1) == S3A_OK);
        CHECK(pair.d == d0 && pair.h == h0 && pair.cap == grow && g_allocs == before);
    }
    /* single-sided ones: pinned with an element size and pad bytes of its own; device only, cleared by hand */
    {
        const int32_t rc = pinned.reserve(m, S3A_GROW_PIN, 5, 1 << 10, 4, 64);
        if (rc != S3A_OK) CHECK(rc == S3A_ENOMEM && !pinned.d && !pinned.h && pinned.cap == 0);
        else CHECK(!pinned.d && pinned.h && g_live[pinned.h] == 2 && g_last_bytes == (size_t)(1 << 10) * 4 + 64);
        const int32_t rc2 = dev.reserve(m, S3A_GROW_DEV, 3, 8, 100);
        if (rc2 != S3A_OK) CHECK(rc2 == S3A_ENOMEM && !dev.d && !dev.h && dev.cap == 0);
        else CHECK(dev.d && !dev.h && g_live[dev.d] == 1 && g_last_bytes == 800);
        dev.clear(m);
        CHECK(!dev.d && dev.cap == 0);
        /* a pinned side with flags of its own */
        const int32_t rc3 = dev.reserve(m, S3A_GROW_PIN, 2, 2, 4, 0, 0x40000000u);
        if (rc3 != S3A_OK) CHECK(rc3 == S3A_ENOMEM && !dev.h && dev.cap == 0);
        else CHECK(dev.h && g_live[dev.h] == 2 && g_last_flags == 0x40000000u && g_last_bytes == 8);
    }
done:
    /* scope exit of an owner with live buffers: the destructor is free_all().  (An owner cannot be copied: it would free twice.) */
    static_assert(!std::is_copy_constructible<s3a_hostmem>::value && !std::is_copy_assignable<s3a_hostmem>::value, "s3a_hostmem must not be copyable");
    {
        s3a_hostmem scoped;
        int32_t *x = NULL;
        void *y = NULL;
        const size_t live0 = g_live.size();
        if (scoped.dev(x, 12) && scoped.pin(y, 12)) CHECK(g_live.size() == live0 + 2);
        else CHECK(g_allocs == fail_at);
        if (g_live.size() == live0) CHECK(scoped.recs.empty());
    }
    CHECK(g_live.size() == m.recs.size());      /* (the scoped owner freed its own, and only its own) */
    m.free_all();
    CHECK(m.recs.empty());
    CHECK(g_live.empty());              /* (nothing leaks, whatever failed) */
    for (auto &kv : g_live) free(kv.first);
    g_live.clear();
    return g_allocs;
}

int
main(void)
{
    const int n = script(0);
    if (n != 17) { fprintf(stderr, "hostmem_check: the script made %d allocations, 17 expected\n", n); return 1; }
    for (int k = 1; k <= n; k++) (void)script(k);
    if (g_bad) { fprintf(stderr, "hostmem_check: %d checks failed\n", g_bad); return 1; }
    printf("hostmem_check: ok (%d allocations, a failure at each in turn)\n", n);
    return 0;
}
