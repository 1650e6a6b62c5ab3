// Bilinear sampling, align_corners = False (PyTorch semantics): the source taps and the sampled value shared by the kernels that return a
// mask to its image (sam_ops.hip: cvmi_bilinear_f32, cvmi_mask_postprocess*, the refinement head; mask_amg.hip: cvmi_amg_score).
#pragma once

// destination index d of an axis resized in -> out with scale = (float)in / (float)out: taps i0, i1 and the weight of i1
__device__ __forceinline__ void bil_axis(int d, float scale, int in, int& i0, int& i1, float& l1) {
  float s = ((float)d + 0.5f) * scale - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
}

__device__ __forceinline__ float bil_sample(const float* __restrict__ pl, int w, int y0, int y1, float ly, int x0, int x1, float lx) {
  const float hy = 1.f - ly, hx = 1.f - lx;
  return hy * (hx * pl[(size_t)y0 * w + x0] + lx * pl[(size_t)y0 * w + x1]) + ly * (hx * pl[(size_t)y1 * w + x0] + lx * pl[(size_t)y1 * w + x1]);
}

// bil_sample's value on four taps already in registers, with the roundings of bilinear_kernel (cvmi_bilinear_f32, cvmi_mask_postprocess)
// WRITTEN OUT.  The expression above leaves the contraction to the compiler, and it does not contract it the same way everywhere: the
// scalar loop of bilinear_kernel gets v_mul + v_fmac for each row and for the final mix, a loop the vectoriser packs gets v_pk_mul and a
// plain add -- one rounding more.  A kernel that must land on the same side of a threshold as the map cvmi_bilinear_f32 writes
// (cvmi_amg_score) therefore states the three fused multiply-adds; tests/test_amg_gpu.py holds the two to the same bits.
__device__ __forceinline__ float bil_mix(float v00, float v01, float v10, float v11, float ly, float lx) {
  const float hy = 1.f - ly, hx = 1.f - lx;
  const float top = fmaf(lx, v01, hx * v00), bot = fmaf(lx, v11, hx * v10);
  return fmaf(hy, top, ly * bot);
}
