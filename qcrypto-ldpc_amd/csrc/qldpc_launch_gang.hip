/*
 * qldpc_launch_gang.hip -- the template instances of the gang layer kernels (qldpc_kernels_gang.h) and the dispatch from a kernel class
 * (degree cap, rule family, explicit messages / compressed check state) to its instance.  A class without an instance is an error, not
 * a fall-back to the members' own launches.
 */
#include "qldpc_engine_int.h"

template <int FAM>
static int launch_gang_fam(hipStream_t stream, int cap, int cst, const qk_gang_args &a, unsigned grid)
{
    if (cst) {
        if constexpr (FAM == QK_FAM_MS || FAM == QK_FAM_AMS) {
            switch (cap) {      /* the bucket of cap 40 holds degrees 21 .. 32 here: the state has one mask bit per edge (qldpc_kernels_cst.h) */
            case 8: hipLaunchKernelGGL((qk_cn_layer_cst_gang<8, FAM>), dim3(grid), dim3(QK_THREADS), 0, stream, a); return QLDPC_OK;
            case 12: hipLaunchKernelGGL((qk_cn_layer_cst_gang<12, FAM>), dim3(grid), dim3(QK_THREADS), 0, stream, a); return QLDPC_OK;
            case 20: hipLaunchKernelGGL((qk_cn_layer_cst_gang<20, FAM>), dim3(grid), dim3(QK_THREADS), 0, stream, a); return QLDPC_OK;
            case 40: hipLaunchKernelGGL((qk_cn_layer_cst_gang<32, FAM>), dim3(grid), dim3(QK_THREADS), 0, stream, a); return QLDPC_OK;
            default: break;
            }
        }
        qldpc_set_error("gang launch: no compressed-state kernel for cap %d, rule family %d", cap, FAM);
        return QLDPC_EUNSUPPORTED;
    }
    switch (cap) {
    case 8: hipLaunchKernelGGL((qk_cn_layer_gang<8, FAM>), dim3(grid), dim3(QK_THREADS), 0, stream, a); return QLDPC_OK;
    case 12: hipLaunchKernelGGL((qk_cn_layer_gang<12, FAM>), dim3(grid), dim3(QK_THREADS), 0, stream, a); return QLDPC_OK;
    case 20: hipLaunchKernelGGL((qk_cn_layer_gang<20, FAM>), dim3(grid), dim3(QK_THREADS), 0, stream, a); return QLDPC_OK;
    case 40: hipLaunchKernelGGL((qk_cn_layer_gang<40, FAM>), dim3(grid), dim3(QK_THREADS), 0, stream, a); return QLDPC_OK;
    case 0: hipLaunchKernelGGL((qk_cn_layer_gang<0, FAM>), dim3(grid), dim3(QK_THREADS), 0, stream, a); return QLDPC_OK;
    default: break;
    }
    qldpc_set_error("gang launch: no kernel for cap %d", cap);
    return QLDPC_EUNSUPPORTED;
}

int qldpc_launch_layer_gang(hipStream_t stream, int cap, int fam, int cst, const qk_gang_args &a, unsigned grid)
{
    switch (fam) {
    case QK_FAM_MS: return launch_gang_fam<QK_FAM_MS>(stream, cap, cst, a, grid);
    case QK_FAM_SPA: return launch_gang_fam<QK_FAM_SPA>(stream, cap, cst, a, grid);
    case QK_FAM_LSPA: return launch_gang_fam<QK_FAM_LSPA>(stream, cap, cst, a, grid);
    default: return launch_gang_fam<QK_FAM_AMS>(stream, cap, cst, a, grid);
    }
}

extern "C" int qldpc_gang_locate_host(const int *prefix, int n, int block, int *member, int *local)
{
    if (!prefix || !member || !local || n < 1 || n > QK_GANG_SLOTS || prefix[0] != 0 || block < 0) { qldpc_set_error("gang_locate_host: bad argument (n in 1..%d, prefix[0] = 0, block >= 0)", QK_GANG_SLOTS); return QLDPC_EINVAL; }
    int p[QK_GANG_SLOTS + 1];
    for (int k = 0; k <= QK_GANG_SLOTS; k++) {
        p[k] = prefix[std::min(k, n)];      /* slots not in use repeat the total, as a launch passes them */
        if (k > 0 && p[k] < p[k - 1]) { qldpc_set_error("gang_locate_host: prefix decreases at %d", k); return QLDPC_EINVAL; }
    }
    int slot, loc;
    qk_gang_locate(p, block, &slot, &loc);
    if (slot >= n) { qldpc_set_error("gang_locate_host: block %d is past the %d blocks of the launch", block, prefix[n]); return QLDPC_EINVAL; }
    *member = slot; *local = loc;
    return QLDPC_OK;
}
