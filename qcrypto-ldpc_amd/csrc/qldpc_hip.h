/*
 * qldpc_hip.h -- the error checks of every HIP translation unit of libqldpc: a failed runtime call or kernel launch leaves its
 * place and HIP's message in qldpc_last_error() and makes the enclosing function return QLDPC_EHIP.
 */
#ifndef QLDPC_HIP_H
#define QLDPC_HIP_H

#include <hip/hip_runtime.h>

#include "../../include/qldpc.h"
#include "qldpc_graph.h"

#define HIPCHK(expr)                                                                                    \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess) {                                                                        \
            qldpc_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__));     \
            return QLDPC_EHIP;                                                                          \
        }                                                                                               \
    } while (0)

#define LAUNCHCHK()                                                                                     \
    do {                                                                                                \
        hipError_t e__ = hipGetLastError();                                                             \
        if (e__ != hipSuccess) { qldpc_set_error("%s:%d: kernel launch -> %s", __FILE__, __LINE__, hipGetErrorString(e__)); return QLDPC_EHIP; } \
    } while (0)

#endif /* QLDPC_HIP_H */
