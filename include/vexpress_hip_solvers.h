/* libvexpress_hip.so — fourth header of the C ABI: solver entry points added after include/vexpress_hip.h was frozen at
 * ABI 15, include/vexpress_hip_guidance.h at its three functions and include/vexpress_hip_samplers.h at its two.  Both
 * libraries (bfloat16 and IEEE-half elements) export them next to the other headers'; the conventions are the first
 * header's (device pointers owned by the caller, asynchronous launches on `stream`, 0 = ok, <0 = VX_ERR_* with the message
 * in vx_last_error_string()).  This header carries its own version, checked by the binding like the others'.
 */
#ifndef VEXPRESS_HIP_SOLVERS_H
#define VEXPRESS_HIP_SOLVERS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VX_SOLVERS_ABI_VERSION 1

int vx_solvers_abi_version(void);

/* ---- One UniPC update per frame (predictor-corrector multistep, data prediction, v-prediction, in the
 * variance-preserving frame of the loop), float32 only: the corrector of the step that ended at this sample and the
 * predictor to the next one, in one launch.  latents, preds, terms, frame_ids, count: as vx_overlap_ddim_step takes them;
 * v is the mean of the terms summed exactly as that kernel sums it.  history: fp32 [3][c, total_frames, hw], each slot laid
 * out like the latents; h1, h2, h3, h_write: slot numbers 0..2, or -1.  saved: fp32 laid out like the latents (the
 * corrected sample of the previous update).  Per element `off` of a frame of frame_ids, with x = latents[off]:
 *     m   = a_i x - s_i v
 *     xc  = use_c ? q_s saved[off] + q_m m + q_1 history[h1][off] + q_2 history[h2][off] + q_3 history[h3][off] : x
 *     out = k_x xc + k_m m + k_1 history[h1][off] + k_2 history[h2][off]
 *     saved[off] = xc
 *     if h_write >= 0: history[h_write][off] = m
 *     latents[off] = out
 * Every read happens before any write: h_write may name one of the slots just read.  A term whose slot is -1 is skipped
 * and its buffer never read (a slot that was never written may hold anything); with use_c == 0 neither saved nor
 * history[h3] is read.  Frames outside frame_ids are not touched in any buffer.  Every product and every sum is one
 * float32 operation, the sums taken left to right as written.
 * Rounding: with T = max_terms the longest path of the expression - a term of v through m and xc into out - carries
 * K = T + 11 roundings (T for its division by count and the sum of the terms; 2 for s_i v and the difference m; 5 for
 * q_m m and the four sums of xc that follow it; 4 for k_x xc and the three sums of out), so
 *     |out - exact| <= (T + 11) 2^-24 sum |terms of the expanded expression|
 * to first order, and likewise (T + 7) for xc and (T + 2) for m.  A contraction to a fused multiply-add only removes
 * roundings.
 * One thread per (frame slot, channel, pixel quad), 16-byte loads and stores: hw % 4 == 0 and 16-byte aligned latents,
 * preds, history and saved.
 * Errors (before any launch, the argument named in the message): a null latents / preds / terms / frame_ids / count /
 * saved, a slot outside -1..2, history == NULL while a slot is >= 0, use_c outside 0..1, hw % 4 != 0, a misaligned
 * pointer, a non-positive extent. */
int vx_overlap_unipc_step(float* latents, int c, int total_frames, int hw, const float* preds, int f_window,
                          const int32_t* terms, int max_terms, const int32_t* frame_ids, const float* count,
                          int n_frames, float* history, int h1, int h2, int h3, int h_write,
                          float* saved, int use_c, float a_i, float s_i,
                          float q_s, float q_m, float q_1, float q_2, float q_3,
                          float k_x, float k_m, float k_1, float k_2, void* stream);

#ifdef __cplusplus
}
#endif
#endif
