/*
 * devmem_sanitize.cc -- the allocation ledger of qcrypto-ldpc_amd/csrc/qldpc_devmem.h on the host, under AddressSanitizer, UBSan and LeakSanitizer
 * (tests/test_devmem_host.py builds and runs it): malloc / free stand behind the two raw hooks, and the k-th raw allocation can be made to fail.
 * Every block is freed by the ledger alone, so a free path that misses one is a leak report, and one that frees twice an ASan report.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>

static int raw_allocs, raw_frees, raw_pinned_live, fail_at;      /* fail_at = k > 0: the k-th raw allocation from now on fails */

static int dm_raw_alloc(void **p, size_t bytes, bool pinned)
{
    if (fail_at > 0 && --fail_at == 0) { *p = nullptr; return 1; }
    *p = malloc(bytes);
    if (!*p) return 1;
    raw_allocs++;
    raw_pinned_live += pinned ? 1 : 0;
    return 0;
}
static void dm_raw_free(void *p, bool pinned)
{
    raw_frees++;
    raw_pinned_live -= pinned ? 1 : 0;
    free(p);
}

#define QLDPC_DEVMEM_HOST_TEST
#include "qldpc_devmem.h"

#define CHECK(cond)                                                                           \
    do {                                                                                      \
        if (!(cond)) { printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static void test_counts(void)
{
    dm_ledger m;
    uint32_t *a = nullptr, *b = nullptr, *c = nullptr, *z = (uint32_t *)0x10, *h = nullptr;
    CHECK(m.dev_bytes == 0 && m.blocks.empty());
    CHECK(dm_alloc(&m, &a, 10) == QLDPC_OK && a && m.dev_bytes == 40);
    a[9] = 1u;                                                       /* exactly sizeof(T) * count bytes: ASan has the byte after */
    CHECK(dm_alloc(&m, &z, 0) == QLDPC_OK && z == nullptr && m.dev_bytes == 40 && m.blocks.size() == 1);
    CHECK(dm_alloc_pinned(&m, &h, 7) == QLDPC_OK && h && m.dev_bytes == 40 && m.blocks.size() == 2 && raw_pinned_live == 1);
    h[6] = 1u;
    uint8_t *bytes = nullptr;
    CHECK(dm_alloc(&m, &bytes, 3) == QLDPC_OK && m.dev_bytes == 43);
    CHECK(dm_alloc(&m, &b, 5) == QLDPC_OK && dm_alloc(&m, &c, 1) == QLDPC_OK && m.dev_bytes == 67 && m.blocks.size() == 5);
    /* from the middle of the list */
    int frees = raw_frees;
    dm_release(&m, &bytes);
    CHECK(bytes == nullptr && m.dev_bytes == 64 && m.blocks.size() == 4 && raw_frees == frees + 1);
    /* a pointer the ledger does not hold: a second name of a, and NULL */
    uint32_t *alias = a + 1, *null = nullptr;
    dm_release(&m, &alias);
    dm_release(&m, &null);
    CHECK(alias == nullptr && null == nullptr && m.dev_bytes == 64 && m.blocks.size() == 4 && raw_frees == frees + 1);
    a[0] = 2u;                                                       /* still there */
    /* a pinned block goes without touching the count */
    dm_release(&m, &h);
    CHECK(h == nullptr && m.dev_bytes == 64 && m.blocks.size() == 3 && raw_pinned_live == 0);
    dm_release(&m, &a);
    CHECK(m.dev_bytes == 24);
    dm_free_all(&m);
    CHECK(m.dev_bytes == 0 && m.blocks.empty());
    frees = raw_frees;
    dm_free_all(&m);                                                 /* twice */
    CHECK(m.dev_bytes == 0 && m.blocks.empty() && raw_frees == frees);
    CHECK(dm_alloc(&m, &a, 2) == QLDPC_OK && m.dev_bytes == 8);      /* and usable after it */
    dm_free_all(&m);
}

static void test_grow(void)
{
    dm_ledger m;
    uint16_t *p = nullptr, *other = nullptr;
    size_t cap = 0;
    CHECK(dm_grow(&m, &p, &cap, 8) == QLDPC_OK && p && cap == 8 && m.dev_bytes == 16);      /* from nothing */
    CHECK(dm_alloc(&m, &other, 1) == QLDPC_OK && m.dev_bytes == 18);
    uint16_t *was = p;
    int frees = raw_frees;
    CHECK(dm_grow(&m, &p, &cap, 8) == QLDPC_OK && dm_grow(&m, &p, &cap, 3) == QLDPC_OK);    /* fits: the same buffer */
    CHECK(p == was && cap == 8 && m.dev_bytes == 18 && raw_frees == frees && m.blocks.size() == 2);
    CHECK(dm_grow(&m, &p, &cap, 20) == QLDPC_OK);                                           /* does not fit: a new one, the old one freed */
    CHECK(p && cap == 20 && m.dev_bytes == 18 + 2 * (20 - 8) && raw_frees == frees + 1 && m.blocks.size() == 2);
    p[19] = 1;
    was = p;
    fail_at = 1;                                                                            /* the allocation fails: everything stands */
    CHECK(dm_grow(&m, &p, &cap, 100) == QLDPC_ENOMEM);
    CHECK(p == was && cap == 20 && m.dev_bytes == 42 && raw_frees == frees + 1 && m.blocks.size() == 2);
    p[19] = 2;
    dm_free_all(&m);
}

/* the sequence of test_fail: four device blocks and a pinned one */
enum { SEQ_ALLOCS = 5 };
static int sequence(dm_ledger *m, void **ptrs)
{
    int rc;
    if ((rc = dm_alloc(m, (uint64_t **)&ptrs[0], 4)) || (rc = dm_alloc(m, (uint8_t **)&ptrs[1], 5)) || (rc = dm_alloc_pinned(m, (int **)&ptrs[2], 6)) ||
        (rc = dm_alloc(m, (float **)&ptrs[3], 7)) || (rc = dm_alloc(m, (uint16_t **)&ptrs[4], 8))) return rc;
    return QLDPC_OK;
}

static void test_fail(void)
{
    const size_t bytes_before[SEQ_ALLOCS + 1] = {0, 32, 37, 37, 65, 81};      /* dev_bytes before the k-th allocation (1-based) */
    for (int k = 1; k <= SEQ_ALLOCS; k++) {
        dm_ledger m;
        void *ptrs[SEQ_ALLOCS];
        for (auto &p : ptrs) p = (void *)0x10;                        /* a failed allocation leaves NULL, not what was there */
        const int allocs = raw_allocs, frees = raw_frees;
        fail_at = k;
        CHECK(sequence(&m, ptrs) == QLDPC_ENOMEM);
        CHECK(fail_at == 0 && ptrs[k - 1] == nullptr);
        CHECK(m.dev_bytes == bytes_before[k - 1] && m.blocks.size() == (size_t)(k - 1) && raw_allocs == allocs + k - 1);
        dm_free_all(&m);                                              /* frees the rest: LeakSanitizer has the last word */
        CHECK(m.dev_bytes == 0 && raw_frees == frees + k - 1 && raw_pinned_live == 0);
    }
    dm_ledger m;
    void *ptrs[SEQ_ALLOCS];
    CHECK(sequence(&m, ptrs) == QLDPC_OK && m.dev_bytes == bytes_before[SEQ_ALLOCS] && m.blocks.size() == SEQ_ALLOCS);
    dm_free_all(&m);
}

static int scoped(int leave_early)
{
    dm_scope tmp;
    uint32_t *a = nullptr, *b = nullptr;
    if (dm_alloc(&tmp.m, &a, 100)) return -1;
    if (leave_early) return 1;                                        /* a returns with the scope */
    if (dm_alloc(&tmp.m, &b, 100)) return -1;
    a[99] = b[99] = 0u;
    return 0;
}

static void test_scope(void)
{
    int frees = raw_frees;
    CHECK(scoped(1) == 1 && raw_frees == frees + 1);
    CHECK(scoped(0) == 0 && raw_frees == frees + 3);
    fail_at = 2;
    CHECK(scoped(0) == -1 && raw_frees == frees + 4);
}

int main(void)
{
    test_counts();
    test_grow();
    test_fail();
    test_scope();
    CHECK(raw_allocs == raw_frees && raw_pinned_live == 0);
    printf("sanitizer pass ok\n");
    return 0;
}
