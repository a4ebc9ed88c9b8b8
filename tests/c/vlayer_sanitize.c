/* Sanitizer pass over the vertical-layered order of the graph layer (no HIP): built with -fsanitize=address,undefined by tests/test_vlayered_host.py */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc.h"
#include "../../qcrypto-ldpc_amd/csrc/qldpc_graph.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #x, qldpc_last_error()); return 1; } } while (0)

/* the exported order is a permutation cut into classes whose VNs share no check */
static int order_ok(const qldpc_code *c, int want_natural)
{
    const int N = qldpc_code_n(c), M = qldpc_code_m(c), k = qldpc_code_vlayer_count(c);
    if (k <= 0) return 0;
    int *order = malloc(sizeof(int) * (size_t)N), *ptr = malloc(sizeof(int) * ((size_t)k + 1)), *cls = malloc(sizeof(int) * (size_t)N);
    int *seen = calloc((size_t)M, sizeof(int));
    int ok = qldpc_code_vlayer_order(c, order, ptr) == want_natural && ptr[0] == 0 && ptr[k] == N;
    for (int v = 0; v < N; v++) cls[v] = -1;
    for (int l = 0; l < k && ok; l++)
        for (int i = ptr[l]; i < ptr[l + 1] && ok; i++) {
            const int v = order[i];
            ok = v >= 0 && v < N && cls[v] < 0;
            if (!ok) break;
            cls[v] = l;
            for (int s = c->vn_ptr[v]; s < c->vn_ptr[v + 1] && ok; s++) { ok = seen[c->vn_chk[s]] != l + 1; seen[c->vn_chk[s]] = l + 1; }
        }
    free(order); free(ptr); free(cls); free(seen);
    return ok;
}

int main(int argc, char **argv)
{
    const char *gold = argc > 1 ? argv[1] : "tests/golden";
    char path[512];
    qldpc_code *c = NULL;
    CHECK(qldpc_code_vlayer_count(NULL) == QLDPC_EINVAL && qldpc_code_vlayer_order(NULL, NULL, NULL) == QLDPC_EINVAL);
    snprintf(path, sizeof(path), "%s/PEGReg504x1008.alist", gold);
    CHECK(qldpc_code_from_alist(path, &c) == QLDPC_OK);
    CHECK(qldpc_code_vlayer_count(c) == 10 && qldpc_code_vlayer_order(c, NULL, NULL) == 1 && order_ok(c, 1));
    qldpc_code_free(c);
    snprintf(path, sizeof(path), "%s/NR_2_3_112.qc", gold);
    CHECK(qldpc_code_from_qc(path, &c) == QLDPC_OK && order_ok(c, 1) && qldpc_code_vlayer_count(c) == 15);
    qldpc_code_free(c);
    CHECK(qldpc_code_from_qc(path, &c) == QLDPC_OK);      /* never asked for its vertical order: nothing built, nothing leaked */
    qldpc_code_free(c);
    CHECK(qldpc_code_ira(65536, 52429, 0.125f, 11, 3, 7, &c) == QLDPC_OK);      /* BASELINE config 2: DSATUR on the VN-conflict graph */
    CHECK(order_ok(c, 0) && qldpc_code_vlayer_count(c) >= qldpc_code_max_cn_degree(c));
    printf("config-2 code: %d vertical classes (max dc %d), %d horizontal layers\n", qldpc_code_vlayer_count(c), qldpc_code_max_cn_degree(c), qldpc_code_layer_count(c));
    qldpc_code_free(c);
    CHECK(qldpc_code_ira(8192, 7373, 0.125f, 11, 3, 7, &c) == QLDPC_OK);        /* rate 0.9: check degree ~ 40, the growing-bitset fall-back may be needed */
    CHECK(order_ok(c, 0) && qldpc_code_vlayer_count(c) >= qldpc_code_max_cn_degree(c));
    printf("rate-0.9 code: %d vertical classes (max dc %d)\n", qldpc_code_vlayer_count(c), qldpc_code_max_cn_degree(c));
    qldpc_code_free(c);
    CHECK(qldpc_code_ira_peg(8192, 6554, 0.125f, 11, 3, 2, 7, &c) == QLDPC_OK && order_ok(c, 0));
    qldpc_code_free(c);
    printf("vertical-layered order: sanitizer pass ok\n");
    return 0;
}
