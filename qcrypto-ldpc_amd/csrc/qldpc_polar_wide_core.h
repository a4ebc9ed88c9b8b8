/*
 * qldpc_polar_wide_core.h -- the memory plan of the WIDE form of the SC decoder of qldpc_polar_*: one workgroup per frame, lanes over the beliefs of
 * a node.  Plain C, shared by the kernel (qldpc_kernels_polar_wide.h) and by the host walk of the plan (qldpc_polar_wide_host.c).  The rules (f, g,
 * the leaf, the two message types, the outputs, the schedule by 32-leaf blocks) are qldpc_polar_core.h's, unchanged; this file only says where a
 * frame's beliefs and partial sums live.  It applies to n >= 6: a frame of n <= 5 is one leaf block and has no level to place.
 *
 *   level n        the input: the frame's row of the caller's llr, read in place (clamped on the way with int8 messages), never copied.
 *   levels n-1 .. C+1   the frame's SCRATCH in device memory, frame-major, each level contiguous, level l (2^l beliefs) at plw_level_off(n, l):
 *                  2^n - 2^(C+1) elements a frame, which is below N.  Level l is produced 2^(n-1-l) times a frame.
 *   levels C .. 6  the workgroup's LDS, level l at plw_lds_off(C, l): 2^(C+1) - 64 elements.  C = plw_chip(n, c) = min(c, n - 1), c the chip
 *                  level asked for (PLW_CHIP_LOG unless the context was told otherwise), 6 <= c <= PLW_CHIP_MAX.
 *   levels 5 .. 0  a leaf block, in registers: leaf t on lane t of the first 32 lanes (or the whole block on one lane, PLW_LEAF_LANES).
 *   u, x rows      [frame][W] words in device memory (the caller's rows where given).  The words of the 64-block window at work (PLW_WIN) stay
 *                  on chip: the decisions, the re-encoded words of the nodes finished inside the window (every combine below 64 words), and the
 *                  window's frozen flags and values.  A full window is written out in one piece, and the combines of 64 words and more run over
 *                  the row in device memory, spread over the lanes.
 *   g's bits       a g at level l <= PLW_WIN_LOG + 4 reads a node of at most 32 words that ends inside the window: from the window.  Above that
 *                  the node ended with an earlier window: from the row.
 */
#ifndef QLDPC_POLAR_WIDE_CORE_H
#define QLDPC_POLAR_WIDE_CORE_H

#include <stddef.h>

#include "qldpc_polar_core.h"

#define PLW_CHIP_LOG 12            /* the default chip level: float messages hold 32 KiB of LDS a workgroup, int8 messages 8 KiB */
#define PLW_CHIP_MIN (PL_SUB_LOG + 1)
#define PLW_CHIP_MAX 13            /* float messages: 64 KiB less 256 bytes */
#define PLW_LANES 256              /* the default workgroup */
#define PLW_LEAF_LANES 32          /* the default lanes of a leaf block: 32, leaf t on lane t, or 0, the whole block on one lane */
#define PLW_WIN_LOG 6
#define PLW_WIN (1 << PLW_WIN_LOG) /* leaf blocks (words of a row) of a window */

/* the lowest level outside the leaf block that a frame of 2^n has is 6, the highest n - 1 */
PL_FN int plw_chip(int n, int c) { return c < n - 1 ? c : n - 1; }
/* levels n-1 .. C+1 in the frame's scratch: the elements before level l, and all of them */
PL_FN size_t plw_level_off(int n, int l) { return ((size_t)1 << n) - ((size_t)2 << l); }
PL_FN size_t plw_scratch_elems(int n, int c) { return n > PL_SUB_LOG ? plw_level_off(n, plw_chip(n, c)) : 0; }
/* levels C .. 6 in LDS (C = plw_chip(n, c)): the elements before level l, and all of them */
PL_FN size_t plw_lds_off(int C, int l) { return ((size_t)2 << C) - ((size_t)2 << l); }
PL_FN size_t plw_lds_elems(int n, int c) { return n > PL_SUB_LOG + 1 ? plw_lds_off(plw_chip(n, c), PL_SUB_LOG) : 0; }
/* words of a window of a row of 2^n bits */
PL_FN size_t plw_win_words(int n) { return n - PL_SUB_LOG < PLW_WIN_LOG ? (size_t)1 << (n - PL_SUB_LOG) : (size_t)PLW_WIN; }
/* does the g that makes level l read its bits from the window? */
PL_FN int plw_g_in_window(int l) { return l <= PLW_WIN_LOG + PL_SUB_LOG - 1; }

#endif /* QLDPC_POLAR_WIDE_CORE_H */
