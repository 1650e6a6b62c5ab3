// (image, prompt) pairs whose images a device table names (`Sam2Plan(pairs=cap)`, `infer_masks` with one prompt list per image): the pass that
// stands where cvmi_repeat_images stands when every image has the same number of prompts.  Built once: a 16-byte copy, the 16-bit copy's type
// is a run-time argument.
//
//   gather_images_kernel   dst[n] = src[pair_image[n]], every 16-byte chunk read once and stored once; optionally the chunk's four f32 values
//                          rounded once to the plan's 16-bit operand type as well (in a 16-bit plan the first cast of the gathered tensor).
#include <algorithm>

#include "common.hpp"

namespace {

constexpr int NT = 256;
constexpr int GRID_CAP = 64;                  // workgroups per pair (repeat_images_kernel's cap); longer images go round the grid-stride loop

template <typename TL> using Lp4 = TL __attribute__((ext_vector_type(4)));        // four 16-bit values: one 8-byte store

template <typename TL>
__global__ __launch_bounds__(NT) void gather_images_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, TL* __restrict__ dst_lp, long long chunks,
                                                           const int* __restrict__ pair_image) {
  // grid.y = pair; the table entry is uniform over the workgroup
  const int n = blockIdx.y;
  const u32x4* s = src + (size_t)pair_image[n] * chunks;
  u32x4* d = dst + (size_t)n * chunks;
  Lp4<TL>* l = dst_lp ? reinterpret_cast<Lp4<TL>*>(dst_lp) + (size_t)n * chunks : nullptr;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < chunks; i += (long long)gridDim.x * NT) {
    const u32x4 v = s[i];
    d[i] = v;
    if (l) {
      const f32x4 f = __builtin_bit_cast(f32x4, v);
      Lp4<TL> o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (TL)f[k];
      l[i] = o;
    }
  }
}

}  // namespace

extern "C" int cvmi_gather_images(const void* src, void* dst, void* dst_lp, int lp_dtype, long long bytes_per_image, const int* pair_image, int n_pairs,
                                  cvmi_stream_t stream_) {
  CVMI_CHECK(src && dst && pair_image && bytes_per_image > 0 && bytes_per_image % 16 == 0 && n_pairs > 0 && n_pairs <= 65535, "gather_images: bad arguments");
  CVMI_CHECK(!dst_lp || lp_dtype == CVMI_F16 || lp_dtype == CVMI_BF16, "gather_images: the 16-bit copy must be CVMI_F16 or CVMI_BF16");
  CVMI_CHECK((((uintptr_t)src | (uintptr_t)dst) & 15) == 0 && ((uintptr_t)dst_lp & 7) == 0 && ((uintptr_t)pair_image & 3) == 0,
             "gather_images: pointers must be 16-byte aligned (the 16-bit copy 8-byte)");
  const long long chunks = bytes_per_image / 16;
  const dim3 g((unsigned)std::min<long long>((chunks + NT - 1) / NT, GRID_CAP), (unsigned)n_pairs), b(NT);
  hipStream_t s = (hipStream_t)stream_;
  if (dst_lp && lp_dtype == CVMI_BF16) {
    cvmi_note_kernel("gather_images_kernel<__bf16>");
    hipLaunchKernelGGL(gather_images_kernel<__bf16>, g, b, 0, s, (const u32x4*)src, (u32x4*)dst, (__bf16*)dst_lp, chunks, pair_image);
  } else {
    cvmi_note_kernel("gather_images_kernel<_Float16>");
    hipLaunchKernelGGL(gather_images_kernel<_Float16>, g, b, 0, s, (const u32x4*)src, (u32x4*)dst, (_Float16*)dst_lp, chunks, pair_image);
  }
  CVMI_LAUNCH_CHECK();
  return 0;
}
