// Sampler kernels declared in include/vexpress_hip_samplers.h: the linear multistep update of the denoising loop
// (vx_overlap_linear_step: Euler discrete, LMS discrete and PNDM/PLMS, all written in the loop's variance-preserving frame).
// float32 only: both element builds carry the same code.
#include "../../include/vexpress_hip_samplers.h"
#include "vx_common.h"
#include "vx_overlap.h"

extern "C" int vx_samplers_abi_version(void) { return VX_SAMPLERS_ABI_VERSION; }

namespace {

// One linear multistep update per frame: the averaged v exactly as overlap_ddim_kernel sums it (mean_of_terms4), then
//   b = saved_mode == 2 ? saved : x;  m = p_x x + p_v v;  out = k_x b + k_v v + c_1 H[h1] + c_2 H[h2] + c_3 H[h3]
// with H the three history slots (each laid out like the latents, `slot_sz` floats apart).  A slot < 0 is skipped and its
// buffer never read; saved_mode == 1 stores x to `saved`; h_write >= 0 stores m to that slot - possibly one just read:
// every thread reads its own 16 bytes of each buffer before it writes them, and no thread touches another's.
// One thread per (frame slot, channel, pixel quad): float4 loads and stores (hw % 4 == 0, 16-byte aligned rows).  The
// slot numbers and saved_mode are kernel arguments, so every branch is uniform over the grid.
__global__ void overlap_linear_kernel(float* latents, int c, int total_frames, int hw, const float* preds, int f_window,
                                      const int32_t* terms, int max_terms, const int32_t* frame_ids, const float* count,
                                      int n_frames, float* history, size_t slot_sz, int h1, int h2, int h3, int h_write,
                                      float* saved, int saved_mode, float k_x, float k_v, float c_1, float c_2,
                                      float c_3, float p_x, float p_v) {
  const int hq = hw >> 2;
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;   // (frame slot, channel, pixel quad)
  long total = (long)n_frames * c * hq;
  if (idx >= total) return;
  int q = (int)(idx % hq);
  int ch = (int)((idx / hq) % c);
  int fs = (int)(idx / ((long)hq * c));
  int fr = frame_ids[fs];
  const float4 v = mean_of_terms4(preds, c, f_window, hw, terms, max_terms, fs, ch, 4 * q, count[fs]);
  const size_t off = ((size_t)ch * total_frames + fr) * hw + 4 * q;
  const float4 x = *reinterpret_cast<const float4*>(latents + off);
  const float4 b = saved_mode == 2 ? *reinterpret_cast<const float4*>(saved + off) : x;
  float4 out;
  out.x = k_x * b.x + k_v * v.x;
  out.y = k_x * b.y + k_v * v.y;
  out.z = k_x * b.z + k_v * v.z;
  out.w = k_x * b.w + k_v * v.w;
  const int hs[3] = {h1, h2, h3};
  const float cs[3] = {c_1, c_2, c_3};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (hs[j] < 0) continue;
    const float4 h = *reinterpret_cast<const float4*>(history + (size_t)hs[j] * slot_sz + off);
    out.x += cs[j] * h.x; out.y += cs[j] * h.y; out.z += cs[j] * h.z; out.w += cs[j] * h.w;
  }
  if (saved_mode == 1) *reinterpret_cast<float4*>(saved + off) = x;
  if (h_write >= 0) {
    float4 m;
    m.x = p_x * x.x + p_v * v.x;
    m.y = p_x * x.y + p_v * v.y;
    m.z = p_x * x.z + p_v * v.z;
    m.w = p_x * x.w + p_v * v.w;
    *reinterpret_cast<float4*>(history + (size_t)h_write * slot_sz + off) = m;
  }
  *reinterpret_cast<float4*>(latents + off) = out;
}

bool slot_ok(int s) { return s >= -1 && s <= 2; }

}  // namespace

extern "C" int vx_overlap_linear_step(float* latents, int c, int total_frames, int hw, const float* preds, int f_window,
                                      const int32_t* terms, int max_terms, const int32_t* frame_ids, const float* count,
                                      int n_frames, float* history, int h1, int h2, int h3, int h_write, float* saved,
                                      int saved_mode, float k_x, float k_v, float c_1, float c_2, float c_3, float p_x,
                                      float p_v, void* stream) {
  VX_REQUIRE(latents, "vx_overlap_linear_step: latents is NULL");
  VX_REQUIRE(preds, "vx_overlap_linear_step: preds is NULL");
  VX_REQUIRE(terms, "vx_overlap_linear_step: terms is NULL");
  VX_REQUIRE(frame_ids, "vx_overlap_linear_step: frame_ids is NULL");
  VX_REQUIRE(count, "vx_overlap_linear_step: count is NULL");
  VX_REQUIRE(c > 0 && total_frames > 0 && hw > 0 && f_window > 0 && max_terms > 0 && n_frames > 0,
             "vx_overlap_linear_step: c, total_frames, hw, f_window, max_terms and n_frames must be positive");
  VX_REQUIRE(hw % 4 == 0, "vx_overlap_linear_step: hw = %d must be a multiple of 4", hw);
  VX_REQUIRE(slot_ok(h1), "vx_overlap_linear_step: h1 = %d outside -1..2", h1);
  VX_REQUIRE(slot_ok(h2), "vx_overlap_linear_step: h2 = %d outside -1..2", h2);
  VX_REQUIRE(slot_ok(h3), "vx_overlap_linear_step: h3 = %d outside -1..2", h3);
  VX_REQUIRE(slot_ok(h_write), "vx_overlap_linear_step: h_write = %d outside -1..2", h_write);
  VX_REQUIRE(history || (h1 < 0 && h2 < 0 && h3 < 0 && h_write < 0),
             "vx_overlap_linear_step: history is NULL while a slot (h1, h2, h3, h_write) is >= 0");
  VX_REQUIRE(saved_mode >= 0 && saved_mode <= 2, "vx_overlap_linear_step: saved_mode = %d outside 0..2", saved_mode);
  VX_REQUIRE(saved || saved_mode == 0, "vx_overlap_linear_step: saved is NULL while saved_mode = %d", saved_mode);
  VX_REQUIRE(((uintptr_t)latents % 16) == 0 && ((uintptr_t)preds % 16) == 0 && ((uintptr_t)history % 16) == 0 &&
                 ((uintptr_t)saved % 16) == 0,
             "vx_overlap_linear_step: latents, preds, history and saved must be 16-byte aligned");
  const long quads = (long)n_frames * c * (hw / 4);
  VX_REQUIRE(quads <= 0x7fffffffL * 256L, "vx_overlap_linear_step: too many elements for one launch");
  hipLaunchKernelGGL(overlap_linear_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     latents, c, total_frames, hw, preds, f_window, terms, max_terms, frame_ids, count, n_frames, history,
                     (size_t)c * total_frames * hw, h1, h2, h3, h_write, saved, saved_mode, k_x, k_v, c_1, c_2, c_3, p_x,
                     p_v);
  return vx_check_launch("vx_overlap_linear_step");
}
