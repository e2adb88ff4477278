/* s3a_hostmem.h -- who owns an engine's device and pinned memory (host code only).
 *
 * No HIP header is included here: hipMalloc / hipHostMalloc / hipFree / hipHostFree and hipSuccess, s3a_set_error and the S3A_* codes
 * are used as the includer declared them (a .hip file: the runtime's; tests/hostmem_check.cc: counting stand-ins).
 * Every request is one allocation call of its own with exactly the bytes asked for, issued when it is asked for: no pool, no padding.
 */
#ifndef S3A_HOSTMEM_H
#define S3A_HOSTMEM_H
#include <stddef.h>
#include <stdint.h>
#include <vector>

/* allocations with their owner's lifetime: recorded when made, freed by free_all() -- which the destructor calls, so a stack-local owner
 * frees a function's temporaries on every return path -- or, the few given back early, by release() */
struct s3a_hostmem {
    struct Rec { void *p; bool pinned; };
    std::vector<Rec> recs;

    s3a_hostmem() {}
    ~s3a_hostmem() { free_all(); }
    s3a_hostmem(const s3a_hostmem &) = delete;
    s3a_hostmem &operator=(const s3a_hostmem &) = delete;

    /* false + s3a_set_error + ptr = NULL when the allocation fails; a request of 0 bytes still allocates 4.  flags: hipHostMalloc's */
    template <class T> bool dev(T *&ptr, size_t bytes) { return get(ptr, bytes, false, 0); }
    template <class T> bool pin(T *&ptr, size_t bytes, unsigned flags = 0) { return get(ptr, bytes, true, flags); }
    /* forgets p without freeing it (it is its new holder's to free); true when it was recorded as pinned memory */
    bool forget(const void *p)
    {
        for (size_t i = recs.size(); i-- > 0;)
            if (recs[i].p == p) { const bool pinned = recs[i].pinned; recs.erase(recs.begin() + (ptrdiff_t)i); return pinned; }
        return false;
    }
    /* frees ptr now and forgets it.  A pointer that was never recorded is DEVICE memory another object handed over */
    template <class T> void release(T *&ptr)
    {
        void *p = (void *)ptr;
        ptr = NULL;
        if (!p) return;
        if (forget(p)) (void)hipHostFree(p); else (void)hipFree(p);
    }
    void free_all()
    {
        for (size_t i = recs.size(); i-- > 0;) { if (recs[i].pinned) (void)hipHostFree(recs[i].p); else (void)hipFree(recs[i].p); }
        recs.clear();
    }
private:
    template <class T> bool get(T *&ptr, size_t bytes, bool pinned, unsigned flags)
    {
        void *p = NULL;
        const size_t n = bytes > 0 ? bytes : 4;
        ptr = NULL;
        if ((pinned ? hipHostMalloc(&p, n, flags) : hipMalloc(&p, n)) != hipSuccess || !p) {
            s3a_set_error("s3a: %s allocation of %zu bytes failed", pinned ? "pinned" : "device", bytes);
            return false;
        }
        recs.push_back({ p, pinned });
        ptr = (T *)p;
        return true;
    }
};

/* a buffer that only grows: a device side, a pinned side, or both, of one capacity (elements).  Plain data: zero is empty. */
enum { S3A_GROW_DEV = 1, S3A_GROW_PIN = 2 };
template <class T>
struct s3a_grow {
    T *d, *h;
    size_t cap;

    void clear(s3a_hostmem &m) { m.release(d); m.release(h); cap = 0; }
    /* need <= cap: nothing moves.  Otherwise the old sides are freed first, then each side asked for gets new_cap elements of `elem`
     * bytes (+ pad bytes), the device side first (pin_flags: the pinned side's hipHostMalloc flags); new_cap is the caller's growth
     * rule.  On failure the buffer is empty, S3A_ENOMEM is returned and the owner's error text stands (the caller may set its own
     * behind it). */
    int32_t reserve(s3a_hostmem &m, int sides, size_t need, size_t new_cap, size_t elem = sizeof(T), size_t pad = 0, unsigned pin_flags = 0)
    {
        if (need <= cap) return S3A_OK;
        clear(m);
        if (((sides & S3A_GROW_DEV) && !m.dev(d, new_cap * elem + pad)) || ((sides & S3A_GROW_PIN) && !m.pin(h, new_cap * elem + pad, pin_flags))) {
            clear(m);
            return S3A_ENOMEM;
        }
        cap = new_cap;
        return S3A_OK;
    }
};
#endif
