// Bilinear sampling, align_corners = False (PyTorch semantics): the source taps and the sampled value shared by the kernels that return a
// mask to its image (resample.hip: cvmi_bilinear_f32, cvmi_mask_postprocess*; mask_amg.hip: cvmi_amg_score) and by the refinement head
// (sam_ops.hip).
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

// The sampled value with its roundings WRITTEN OUT: three fused multiply-adds on two products.  Every kernel whose value is compared with a
// threshold goes through this one -- the four forms of the mask return and cvmi_amg_score -- so that a pixel lands on the same side of the
// threshold whichever of them resamples the plane (tests/test_resample_bits_gpu.py, tests/test_amg_gpu.py hold them to the same bits).
__device__ __forceinline__ float bil_mix(float v00, float v01, float v10, float v11, float ly, float lx) {
  const float hy = 1.f - ly, hx = 1.f - lx;
  const float top = fmaf(lx, v01, hx * v00), bot = fmaf(lx, v11, hx * v10);
  return fmaf(hy, top, ly * bot);
}

// The refinement head's sample (sam_ops.hip: upsample_refine*), and only its: the expression leaves the contraction to the compiler, which
// does not contract it the same way everywhere (a scalar loop gets v_mul + v_fmac for each row and for the final mix, a loop the vectoriser
// packs gets v_pk_mul and a plain add -- one rounding more).  The head's output feeds convolutions, not a threshold, and is held to fp64 by a
// tolerance; nothing that must agree bit for bit with another kernel may use it.
__device__ __forceinline__ float bil_sample(const float* __restrict__ pl, int w, int y0, int y1, float ly, int x0, int x1, float lx) {
  const float hy = 1.f - ly, hx = 1.f - lx;
  return hy * (hx * pl[(size_t)y0 * w + x0] + lx * pl[(size_t)y0 * w + x1]) + ly * (hx * pl[(size_t)y1 * w + x0] + lx * pl[(size_t)y1 * w + x1]);
}
