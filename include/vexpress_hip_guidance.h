/* libvexpress_hip.so — second header of the C ABI: guidance entry points added after include/vexpress_hip.h was frozen at
 * ABI 15.  Both libraries (bfloat16 and IEEE-half elements) export them next to the first header's; the conventions are
 * that header's (device pointers owned by the caller, asynchronous launches on `stream`, 0 = ok, <0 = VX_ERR_* with the
 * message in vx_last_error_string()).  This header carries its own version, checked by the binding like the first one's.
 */
#ifndef VEXPRESS_HIP_GUIDANCE_H
#define VEXPRESS_HIP_GUIDANCE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VX_GUIDANCE_ABI_VERSION 1

int vx_guidance_abi_version(void);

/* ---- Adaptive projected guidance (Sadat, Hilliges, Weber: "Eliminating Oversaturation and Artifacts of High Guidance
 * Scales in Diffusion Models", ICLR 2025; diffusers' AdaptiveProjectedGuidance), on the model output, float32 only.
 * gathered / unit_index: as vx_combine_units (rows = 2: the rows (u, c) or (m, c) of a window, one scale `guidance`) and
 * vx_combine_units3 (rows = 3: (u, m, c), `guidance` on m - u and `audio_guidance` on c - m) take them; preds fp32
 * [n_windows, c, f, hw].  Per window and per frame slot, over the c * hw values of that frame, for each difference
 * d = (next row) - (row) with its scale s:
 *     dbar = d + momentum * dbar_prev        (stored to momentum_buf, which starts as zeros)
 *     phi  = norm_threshold > 0 and S_dd > 0 ? min(1, norm_threshold / sqrt(S_dd)) : 1,   k = S_cc > 0 ? S_dc / S_cc : 0
 *     A = (s - 1) phi,  B = (s - 1) phi (1 - eta) k          (double, each rounded to float32 once)
 * with S_dd, S_dc, S_cc = sum dbar^2, sum dbar c, sum c^2 (c the last row), and
 *     preds = (c + A1 dbar1) - B1 c                                  rows = 2
 *     preds = (((c + A1 dbar1) - B1 c) + A2 dbar2) - B2 c            rows = 3
 * every product and every sum rounded to float32 on its own (never contracted to an fma).  A frame's result does not
 * depend on the other frames of its window, on how the units are laid out, or on n_windows.
 * Two launches.  (1) one block per (window, frame slot, chunk of 256 pixels) forms dbar (and stores it when
 * momentum != 0) and writes its partial sums - 2 (rows - 1) + 1 floats - to its own place of `workspace`; (2) the same
 * partition merges a frame's partials in ascending chunk order in double, forms A and B and writes preds.  No atomics.
 * momentum_buf: fp32 [rows - 1][n_windows, c, f, hw], read and rewritten in place; NULL if and only if momentum == 0.
 * workspace: fp32, at least vx_guidance_apg_ws_floats(n_windows, rows, f, hw) elements, contents irrelevant.
 * Errors (before any launch, the argument named in the message): rows other than 2 or 3, eta outside [0, 1],
 * norm_threshold negative or not finite, |momentum| >= 1, a short workspace, momentum_buf not matching momentum. */
int64_t vx_guidance_apg_ws_floats(int n_windows, int rows, int f, int hw);
int vx_guidance_apg(const float* gathered, const int32_t* unit_index, int n_windows, int rows, int shards, int c, int f,
                    int hw, float guidance, float audio_guidance, float eta, float norm_threshold, float momentum,
                    float* momentum_buf, float* workspace, int64_t ws_floats, float* preds, void* stream);

#ifdef __cplusplus
}
#endif
#endif
