/* libvexpress_hip.so — third header of the C ABI: sampler entry points added after include/vexpress_hip.h was frozen at
 * ABI 15 and include/vexpress_hip_guidance.h at its three functions.  Both libraries (bfloat16 and IEEE-half elements)
 * export them next to the other headers'; the conventions are the first header's (device pointers owned by the caller,
 * asynchronous launches on `stream`, 0 = ok, <0 = VX_ERR_* with the message in vx_last_error_string()).  This header
 * carries its own version, checked by the binding like the others'.
 */
#ifndef VEXPRESS_HIP_SAMPLERS_H
#define VEXPRESS_HIP_SAMPLERS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VX_SAMPLERS_ABI_VERSION 1

int vx_samplers_abi_version(void);

/* ---- One linear multistep update per frame (Euler discrete, LMS discrete, PNDM/PLMS in the variance-preserving frame of
 * the loop; v-prediction), float32 only.  latents, preds, terms, frame_ids, count: as vx_overlap_ddim_step takes them; v is
 * the mean of the terms summed exactly as that kernel sums it.  history: fp32 [3][c, total_frames, hw], each slot laid
 * out like the latents; h1, h2, h3, h_write: slot numbers 0..2, or -1.  saved: fp32 laid out like the latents.  Per
 * element `off` of a frame of frame_ids, with x = latents[off]:
 *     b   = saved_mode == 2 ? saved[off] : x
 *     m   = p_x x + p_v v
 *     out = k_x b + k_v v + c_1 history[h1][off] + c_2 history[h2][off] + c_3 history[h3][off]
 *     if saved_mode == 1: saved[off] = x
 *     if h_write >= 0:    history[h_write][off] = m
 *     latents[off] = out
 * A term whose slot is -1 is skipped and its buffer never read (a slot that was never written may hold anything);
 * h_write may name one of the slots just read.  Frames outside frame_ids are not touched in any buffer.
 * One thread per (frame slot, channel, pixel quad), 16-byte loads and stores: hw % 4 == 0 and 16-byte aligned latents,
 * preds, history and saved.
 * Errors (before any launch, the argument named in the message): a null latents / preds / terms / frame_ids / count, a
 * slot outside -1..2, history == NULL while a slot is >= 0, saved_mode outside 0..2, saved == NULL while saved_mode != 0,
 * hw % 4 != 0, a misaligned pointer, a non-positive extent. */
int vx_overlap_linear_step(float* latents, int c, int total_frames, int hw, const float* preds, int f_window,
                           const int32_t* terms, int max_terms, const int32_t* frame_ids, const float* count,
                           int n_frames, float* history, int h1, int h2, int h3, int h_write,
                           float* saved, int saved_mode,
                           float k_x, float k_v, float c_1, float c_2, float c_3, float p_x, float p_v, void* stream);

#ifdef __cplusplus
}
#endif
#endif
