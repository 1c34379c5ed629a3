// The guided prediction of a window's rows, shared by every launch that forms it (vx_elem.hip: vx_combine_units,
// vx_combine_units3, vx_guidance_rescale*; vx_reuse.hip: vx_combine_units_keep), so that they agree by construction.
#pragma once
#include "vx_common.h"

// g = u + s (cnd - u), and for three-row guidance (a separate audio scale) g = u + s (m - u) + s_audio (c - m) over the rows
// (u, m, c) of a window - u without any condition, m ("silent") with the reference bank and the keypoints but all-zero audio,
// c with everything - evaluated as cfg_mix(u, m, s) + s_audio * (c - m): where c and m hold equal bits this is the two-row
// u + s (m - u).
__device__ __forceinline__ float cfg_mix(float u, float cnd, float guidance) { return u + guidance * (cnd - u); }

__device__ __forceinline__ float cfg_mix3(float u, float m, float cnd, float guidance, float audio) {
  return cfg_mix(u, m, guidance) + audio * (cnd - m);
}

// the guided prediction at one element of a window's rows: rows[0] = u, rows[ROWS - 1] = c, and rows[1] = m for ROWS = 3.
// ROWS = 1 (no guidance) evaluates u + s (u - u) like the others: -0.0 comes out as +0.0 and an infinity as NaN
template <int ROWS>
__device__ __forceinline__ float guided_value(const float* const* rows, long i, float guidance, float audio) {
  if constexpr (ROWS == 3) return cfg_mix3(rows[0][i], rows[1][i], rows[2][i], guidance, audio);
  else return cfg_mix(rows[0][i], rows[ROWS - 1][i], guidance);
}
