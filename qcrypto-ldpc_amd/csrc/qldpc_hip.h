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

/*
 * The stream switch of every context (decoder, gang member, polar, QBER estimator; qldpc.h "stream switch"): *cur becomes `next`, and what the
 * context has queued on the old stream comes first -- an event recorded on the old stream that `next` waits for, so the call itself waits for
 * nothing.  The same stream again does nothing at all.  The old stream must still exist.  The caller has set the device.
 */
static inline int qldpc_stream_switch(hipStream_t *cur, void *next)
{
    hipStream_t to = (hipStream_t)next;
    if (to == *cur) return QLDPC_OK;
    hipEvent_t ev = nullptr;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, *cur);
    if (e == hipSuccess) e = hipStreamWaitEvent(to, ev, 0);
    (void)hipEventDestroy(ev);      /* released once it has completed: the wait queued above keeps its place */
    HIPCHK(e);
    *cur = to;
    return QLDPC_OK;
}

#endif /* QLDPC_HIP_H */
