/* libvexpress_hip.so — sixth header of the C ABI: the latent resize of two-pass (hi-res) sampling, added without
 * touching include/vexpress_hip.h, include/vexpress_hip_guidance.h, include/vexpress_hip_samplers.h,
 * include/vexpress_hip_solvers.h or include/vexpress_hip_reuse.h.  Both libraries (bfloat16 and IEEE-half elements) export
 * it next to the others'; the conventions are the first header's (device pointers owned by the caller, asynchronous
 * launches on `stream`, 0 = ok, <0 = VX_ERR_* with the message in vx_last_error_string()).  This header carries its own
 * version, checked by the binding like the others'.
 */
#ifndef VEXPRESS_HIP_RESIZE_H
#define VEXPRESS_HIP_RESIZE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VX_RESIZE_ABI_VERSION 1

int vx_resize_abi_version(void);

/* ---- Latent resize: `planes` float32 planes [h, w] -> [h2, w2] (the latents [1, C, F, h, w] are C * F planes), separable,
 * from per-axis tap tables the caller resolved on the host in float64 (torch.nn.functional.interpolate's
 * align_corners=False, antialias=False coordinates; ops.latent_resize builds them): the kernel does no coordinate
 * arithmetic.  iy int32 / wy fp32 [h2, taps]: the source rows of output row y and their weights; ix / wx [w2, taps]: the
 * same for the columns; taps = 2 (bilinear) or 4 (bicubic).  Indices must lie in [0, h - 1] / [0, w - 1] (the kernel clamps
 * what it reads once more, so a bad table cannot reach outside src).  Evaluated in this order, every product and every
 * sum rounded to float32 on its own (never contracted to an fma), so that a float32 host expression gives the same bits:
 *     r_a = wx[x][0] * src[iy[y][a]][ix[x][0]];   r_a = r_a + wx[x][b] * src[iy[y][a]][ix[x][b]]   (b = 1 .. taps - 1)
 *     out = wy[y][0] * r_0;                       out = out + wy[y][a] * r_a                       (a = 1 .. taps - 1)
 * One launch, one thread per (plane, output row, quad of output columns); 16-byte stores where a quad is whole and
 * aligned, scalar stores otherwise (the tail of a row, rows of a width that is no multiple of 4).  No atomics, no
 * workspace.  src and the tables are read only; dst may not alias src.
 * Errors (before any launch, the argument named in the message): a missing buffer, src == dst, a size that is not
 * positive, taps other than 2 or 4. */
int vx_latent_resize(const float* src, int planes, int h, int w, float* dst, int h2, int w2, const int32_t* iy,
                     const float* wy, const int32_t* ix, const float* wx, int taps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
