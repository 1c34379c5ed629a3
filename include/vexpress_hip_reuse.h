/* libvexpress_hip.so — fifth header of the C ABI: the guidance-reuse entry points, added without touching
 * include/vexpress_hip.h, include/vexpress_hip_guidance.h, include/vexpress_hip_samplers.h or
 * include/vexpress_hip_solvers.h.  Both libraries (bfloat16 and IEEE-half elements) export them next to the others'; the
 * conventions are the first header's (device pointers owned by the caller, asynchronous launches on `stream`, 0 = ok,
 * <0 = VX_ERR_* with the message in vx_last_error_string()).  This header carries its own version, checked by the binding
 * like the others'.
 */
#ifndef VEXPRESS_HIP_REUSE_H
#define VEXPRESS_HIP_REUSE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VX_REUSE_ABI_VERSION 1

int vx_reuse_abi_version(void);

/* ---- Guidance reuse (known as CFG-cache; FasterCache's CFG branch without its frequency split): the differences of a
 * window's rows are formed on a refresh step and added to the conditional row alone on the steps between.  float32 only.
 *
 * vx_combine_units_keep: the combine of a refresh step.  gathered / unit_index [n_windows, rows, shards] as
 * vx_combine_units (rows = 2: the rows (u, c) or (m, c) of a window, one scale `guidance`; audio_guidance is not read)
 * and vx_combine_units3 (rows = 3: (u, m, c), `guidance` on m - u and `audio_guidance` on c - m) take them.  preds fp32
 * [n_windows, c, f, hw] holds the bits those two entry points write (the same device functions form it).  diffs fp32
 * [rows - 1][n_windows, c, f, hw]: difference k is (row k + 1) - (row k), one float32 subtraction.  One launch, one
 * thread per (window, frame slot, pixel) looping over the channels; no atomics, no workspace.
 * Errors (before any launch, the argument named in the message): rows other than 2 or 3, a missing buffer, a geometry
 * that is not positive or f not a multiple of shards, a scale that is not finite. */
int vx_combine_units_keep(const float* gathered, const int32_t* unit_index, int n_windows, int rows, int shards, int c,
                          int f, int hw, float guidance, float audio_guidance, float* diffs, float* preds, void* stream);

/* vx_combine_reused: the combine of a reuse step.  gathered / unit_index [n_windows, 1, shards]: the conditional row c
 * alone, as an unguided step gathers it.  last, prev: fp32 [n_diffs][n_windows, c, f, hw], the differences L stored at
 * the last refresh and P at the one before it; prev is NULL if and only if b1 == 0 and b2 == 0 (a2, b2 are not read for
 * n_diffs = 1, and must be 0 there).  preds fp32 [n_windows, c, f, hw], evaluated in this order:
 *     p = c + a1 L1;   p = p + b1 P1 (prev given);   p = p + a2 L2 (n_diffs = 2);   p = p + b2 P2 (n_diffs = 2, prev given)
 * every product and every sum rounded to float32 on its own (never contracted to an fma).  One launch, the partition of
 * vx_combine_units_keep; no atomics, no workspace.  preds may not alias last or prev.
 * Errors (before any launch, the argument named in the message): n_diffs other than 1 or 2, a missing buffer, a bad
 * geometry, a coefficient that is not finite, prev not matching b1 / b2, a2 / b2 not 0 for n_diffs = 1. */
int vx_combine_reused(const float* gathered, const int32_t* unit_index, int n_windows, int n_diffs, int shards, int c,
                      int f, int hw, const float* last, const float* prev, float a1, float b1, float a2, float b2,
                      float* preds, void* stream);

#ifdef __cplusplus
}
#endif
#endif
