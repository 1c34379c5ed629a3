// The mean of the overlapping window predictions, as every update kernel of the denoising loop sums it (vx_elem.hip's
// vx_overlap_*_step, vx_sampler.hip's vx_overlap_linear_step): one statement, so that "summed exactly as
// overlap_ddim_kernel sums it" holds by construction.
#pragma once
#include "vx_common.h"

// The mean of the overlapping predictions of frame slot fs at (ch, px): the reference divides each window's prediction by
// the coverage count BEFORE summing (:553, :556-564); the first valid term initialises the sum, slot < 0 = skip.  The float4
// form is the same per component (px = the first pixel of the quad, 16-byte aligned rows).
__device__ __forceinline__ float mean_of_terms(const float* preds, int c, int f_window, int hw, const int32_t* terms,
                                               int max_terms, int fs, int ch, int px, float ic) {
  float v = 0.f;
  bool first = true;
  for (int t = 0; t < max_terms; ++t) {
    int slot = terms[(fs * max_terms + t) * 2 + 0];
    int li = terms[(fs * max_terms + t) * 2 + 1];
    if (slot < 0) continue;
    float term = preds[(((size_t)slot * c + ch) * f_window + li) * hw + px] / ic;
    v = first ? term : v + term;
    first = false;
  }
  return v;
}

__device__ __forceinline__ float4 mean_of_terms4(const float* preds, int c, int f_window, int hw, const int32_t* terms,
                                                 int max_terms, int fs, int ch, int px, float ic) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  bool first = true;
  for (int t = 0; t < max_terms; ++t) {
    int slot = terms[(fs * max_terms + t) * 2 + 0];
    int li = terms[(fs * max_terms + t) * 2 + 1];
    if (slot < 0) continue;
    const float4 p = *reinterpret_cast<const float4*>(preds + (((size_t)slot * c + ch) * f_window + li) * hw + px);
    const float4 term = make_float4(p.x / ic, p.y / ic, p.z / ic, p.w / ic);
    if (first) {
      v = term;
    } else {
      v.x = v.x + term.x; v.y = v.y + term.y; v.z = v.z + term.z; v.w = v.w + term.w;
    }
    first = false;
  }
  return v;
}
