/*
 * qldpc_devmem.h -- the allocation ledger of every context of libqldpc (host code, not part of the C ABI).  An owner object holds one dm_ledger
 * and allocates everything it owns through it; its *_device_bytes getter reads dev_bytes.  The rules, stated here once:
 *
 *  - dm_alloc allocates exactly sizeof(T) * count bytes of device memory.  A count of zero allocates nothing, leaves *p NULL and succeeds; an
 *    owner that wants one element for an empty array says so at its call.
 *  - dm_alloc, dm_alloc_pinned and dm_grow return QLDPC_OK or QLDPC_ENOMEM.  On failure *p is NULL (dm_grow: unchanged), the ledger and dev_bytes
 *    are as they were, and HIP's sticky error is cleared, so that a later launch check does not report a stale out-of-memory error.  The ledger
 *    writes no error text: the caller words the failure.
 *  - dev_bytes counts device blocks only.  Pinned host blocks are listed, so that dm_free_all frees them, and are not counted.
 *  - dm_grow leaves a buffer that holds count elements alone.  Otherwise it allocates the new block first and then releases the old one: a
 *    failed grow leaves the old buffer, *cap and the byte count standing.  The contents are not copied, and the caller has made sure that nothing
 *    queued still reads the old buffer.
 *  - dm_release takes one block out and frees it; a pointer the ledger does not hold (a second name of a block, or NULL) is only cleared.
 *  - dm_free_all frees what the ledger still holds, the latest block first, and may be called again.
 *  - The ledger selects no device and waits for nothing: an owner keeps its own "set device, wait for the stream, then free" sequence.
 *  - A ledger belongs to one owner object and is touched only by the thread that owns that object.
 *
 * dm_scope is the ledger of a call that allocates temporaries: they are freed on every return.
 *
 * With QLDPC_DEVMEM_HOST_TEST defined before the include, the header does not include HIP and takes dm_raw_alloc(void **, size_t, bool pinned)
 * (0 on success) and dm_raw_free(void *, bool pinned) from the including file (the sanitizer program of the CPU suite).
 */
#ifndef QLDPC_DEVMEM_H
#define QLDPC_DEVMEM_H

#include <cstddef>
#include <vector>

#include "../../include/qldpc.h"

#ifndef QLDPC_DEVMEM_HOST_TEST
#include <hip/hip_runtime.h>

static inline int dm_raw_alloc(void **p, size_t bytes, bool pinned, unsigned flags)
{
    if ((pinned ? hipHostMalloc(p, bytes, flags) : hipMalloc(p, bytes)) == hipSuccess) return 0;
    (void)hipGetLastError();
    return 1;
}
static inline void dm_raw_free(void *p, bool pinned) { (void)(pinned ? hipHostFree(p) : hipFree(p)); }
#define DM_RAW_ALLOC(p, bytes, pinned, flags) dm_raw_alloc(p, bytes, pinned, flags)
#define DM_PINNED_DEFAULT hipHostMallocDefault
#else
#define DM_RAW_ALLOC(p, bytes, pinned, flags) ((void)(flags), dm_raw_alloc(p, bytes, pinned))
#define DM_PINNED_DEFAULT 0u
#endif

/* hidden: the std::vector instances over it stay out of the library's dynamic symbols */
struct __attribute__((visibility("hidden"))) dm_block { void *p; size_t bytes; bool pinned; };
struct __attribute__((visibility("hidden"))) dm_ledger { std::vector<dm_block> blocks; size_t dev_bytes = 0; };

static inline int dm_enter(dm_ledger *m, void **p, size_t bytes, bool pinned, unsigned flags)
{
    *p = nullptr;
    if (bytes == 0) return QLDPC_OK;
    m->blocks.reserve(m->blocks.size() + 1);      /* before the allocation: the push_back below cannot fail */
    if (DM_RAW_ALLOC(p, bytes, pinned, flags)) { *p = nullptr; return QLDPC_ENOMEM; }
    m->blocks.push_back(dm_block{*p, bytes, pinned});
    if (!pinned) m->dev_bytes += bytes;
    return QLDPC_OK;
}

template <class T> static int dm_alloc(dm_ledger *m, T **p, size_t count) { return dm_enter(m, (void **)p, sizeof(T) * count, false, 0); }

template <class T> static int dm_alloc_pinned(dm_ledger *m, T **p, size_t count, unsigned flags = DM_PINNED_DEFAULT)
{
    return dm_enter(m, (void **)p, sizeof(T) * count, true, flags);
}

template <class T> static void dm_release(dm_ledger *m, T **p)
{
    for (auto it = m->blocks.begin(); *p && it != m->blocks.end(); ++it)
        if (it->p == (void *)*p) {
            dm_raw_free(it->p, it->pinned);
            if (!it->pinned) m->dev_bytes -= it->bytes;
            m->blocks.erase(it);
            break;
        }
    *p = nullptr;
}

template <class T> static int dm_grow(dm_ledger *m, T **p, size_t *cap, size_t count)
{
    if (count <= *cap) return QLDPC_OK;
    T *q = nullptr, *old = *p;
    if (int rc = dm_alloc(m, &q, count)) return rc;
    dm_release(m, &old);
    *p = q;
    *cap = count;
    return QLDPC_OK;
}

static inline void dm_free_all(dm_ledger *m)
{
    for (auto it = m->blocks.rbegin(); it != m->blocks.rend(); ++it) dm_raw_free(it->p, it->pinned);
    m->blocks.clear();
    m->dev_bytes = 0;
}

struct __attribute__((visibility("hidden"))) dm_scope { dm_ledger m; ~dm_scope() { dm_free_all(&m); } };

#endif /* QLDPC_DEVMEM_H */
