// Mask prompts and multimask output of the SAM 2 prompt encoder / mask decoder (upstream PromptEncoder._embed_masks, SAM2ImagePredictor._predict
// with mask_input / multimask_output=True).  Built once: f32 arithmetic, the 16-bit copy's type is a run-time argument.
//
//   mask_prompt_embed_kernel   keys[i] = emb[i / rep] + mask_downscaling(mask[i]) - no_mask_embed for the B * rep (image, prompt) pairs, plus the
//                              same values rounded once to the plan's 16-bit operand type.  One launch in the place of cvmi_repeat_images (and,
//                              in 16-bit plans, of layer 0's cast of the image stream).  mask_downscaling is
//                              Conv2d(1, 4, 2, 2) -> LayerNorm2d -> GELU -> Conv2d(4, 16, 2, 2) -> LayerNorm2d -> GELU -> Conv2d(16, 256, 1):
//                              an output pixel reads a 4 x 4 patch of the mask and writes 256 channels, so the kernel is bound by its stores
//                              (1 KiB of f32 + 512 B of 16-bit values per pixel next to 64 B read) and is laid out for them: a wave takes 64
//                              pixels, lane i computes the 16 hidden values of pixel i in registers, then the wave walks its pixels with the
//                              hidden vector of pixel j read across lanes (v_readlane), every lane producing ITS four output channels from the
//                              64 weights of the 1 x 1 convolution it keeps in registers -- one 16-byte store per lane and pixel row.
//                              cvmi_mask_prompt_embed_pairs runs the same kernel for pairs whose images a device table names (prompt lists:
//                              pair i belongs to image pair_image[i] instead of i / rep).
//   multimask_out_kernel       the multimask tail: tokens 1..3 of masks4 / iou4 as contiguous [n, 3, P] / [n, 3] (sibling of select_mask_kernel).
//   best_candidate_kernel      mask feedback between two decoder passes (upstream's recipe for ambiguous prompts): per pair the logits of the
//                              candidate with the highest predicted IoU, copied to the next pass's mask_in.  Every workgroup of a pair reads the
//                              pair's NM IoUs itself (12 bytes, no second launch, no atomics) and then moves 16 bytes per lane and step of the
//                              ONE selected plane: n * P * 4 bytes in, as many out.
//   m2m_fanout_kernel          the mask-to-mask pass of upstream's automatic mask generator: EVERY candidate of a pass becomes a prompt of the
//                              next, single-mask pass.  The pair's NM planes are contiguous on both sides (candidate-major inside the pair), so
//                              the planes are one elementwise torch.clamp (comparisons: a NaN stays) at 16 bytes per lane and step of a
//                              grid-stride loop -- n * NM * P * 4 bytes in, as many out --, and the pair's first workgroup writes its rows of
//                              the prompt tables NM times.  Plain vector stores, no atomics.
#include <algorithm>

#include "common.hpp"

namespace {

constexpr int NT = 256, WAVES = NT / 64;
// packed mask_downscaling (include/cvmi355.h CVMI_MASK_PROMPT_PARAMS floats)
constexpr int O_W1 = 0, O_B1 = 16, O_G1 = 20, O_BE1 = 24, O_W2 = 28, O_B2 = 284, O_G2 = 300, O_BE2 = 316, O_W3 = 332, O_B3 = 4428, N_PARAMS = 4684;
static_assert(N_PARAMS == CVMI_MASK_PROMPT_PARAMS && O_B3 + 256 == N_PARAMS, "layout of the packed mask_downscaling parameters");
constexpr int GRID_CAP = 768;                 // workgroups: 3 per CU (161 VGPRs: 3 waves per SIMD); larger problems go round the grid-stride loop

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

// LayerNorm2d over the C channel values of one pixel (biased variance, eps inside the root) followed by exact GELU
template <int C> __device__ __forceinline__ void ln_gelu(float* a, const float* __restrict__ g, const float* __restrict__ be) {
  float u = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) u += a[c];
  u *= 1.0f / C;
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) { a[c] -= u; s = fmaf(a[c], a[c], s); }
  const float r = 1.0f / sqrtf(s * (1.0f / C) + 1e-6f);
#pragma unroll
  for (int c = 0; c < C; ++c) a[c] = gelu_erf(fmaf(a[c] * r, g[c], be[c]));
}

template <typename TL> using Lp4 = TL __attribute__((ext_vector_type(4)));        // four 16-bit values: one 8-byte store

template <typename TL>
__global__ __launch_bounds__(NT) void mask_prompt_embed_kernel(const float* __restrict__ mask, const float* __restrict__ emb, const float* __restrict__ params,
                                                               float* __restrict__ keys, TL* __restrict__ keys_lp, int rep, int fs, int total,
                                                               const int* __restrict__ pair_image) {
  __shared__ __attribute__((aligned(16))) float prm[N_PARAMS];
  for (int i = threadIdx.x; i < N_PARAMS / 4; i += NT) ((f32x4*)prm)[i] = ((const f32x4*)params)[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // this lane's four output channels 4 * lane .. 4 * lane + 3 of the 1 x 1 convolution: w3[c][0..15] and b3' stay in registers
  float w[4][16], b3[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int m = 0; m < 16; m += 4) {
      const f32x4 t = *(const f32x4*)(prm + O_W3 + (lane * 4 + k) * 16 + m);
      w[k][m] = t[0]; w[k][m + 1] = t[1]; w[k][m + 2] = t[2]; w[k][m + 3] = t[3];
    }
    b3[k] = prm[O_B3 + lane * 4 + k];
  }
  const int P = fs * fs, mw = 4 * fs;                                    // pixels per pair; width of a mask row
  const int groups = (total + 63) / 64;                                  // (total < 2^31 - 64: checked by the launcher)
  for (int g = blockIdx.x * WAVES + wave; g < groups; g += gridDim.x * WAVES) {
    // the small weights are re-read from LDS (uniform addresses: broadcasts) in every round: hoisted out of this loop as the loop invariants
    // they are, they would sit in 332 more registers next to the 68 of w / b3 (measured: 512 registers, one wave per SIMD)
    asm volatile("" ::: "memory");
    const int q0 = g * 64;
    const int cnt = min(64, total - q0);                                 // wave-uniform; the lanes past it recompute the last pixel and store nothing
    const int q = q0 + (lane < cnt ? lane : cnt - 1);
    const int pair = q / P, p = q - pair * P, y = p / fs, x = p - y * fs;
    const int erow = (pair_image ? pair_image[pair] : pair / rep) * P + p;      // row of emb [B * P, 256] this pixel adds (image-major pairs, or the table's image)
    // ---- the 4 x 4 patch -> 4 channels on 2 x 2 -> 16 channels, all in registers
    const float* mp = mask + ((size_t)pair * mw + 4 * y) * mw + 4 * x;
    f32x4 pt[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pt[r] = *(const f32x4*)(mp + (size_t)r * mw);
    float h1[4][2][2];                                                   // [channel][sy][sx]
#pragma unroll
    for (int sy = 0; sy < 2; ++sy)
#pragma unroll
      for (int sx = 0; sx < 2; ++sx) {
        float a[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float v = prm[O_B1 + c];
#pragma unroll
          for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) v = fmaf(prm[O_W1 + (c * 2 + dy) * 2 + dx], pt[2 * sy + dy][2 * sx + dx], v);
          a[c] = v;
        }
        ln_gelu<4>(a, prm + O_G1, prm + O_BE1);
#pragma unroll
        for (int c = 0; c < 4; ++c) h1[c][sy][sx] = a[c];
      }
    float h[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) {
      float v = prm[O_B2 + o];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
          for (int dx = 0; dx < 2; ++dx) v = fmaf(prm[O_W2 + ((o * 4 + c) * 2 + dy) * 2 + dx], h1[c][dy][dx], v);
      h[o] = v;
    }
    ln_gelu<16>(h, prm + O_G2, prm + O_BE2);
    // ---- the walk: pixel j's hidden vector to every lane, 4 channels per lane, one 16-byte store per lane and row
    for (int j = 0; j < cnt; ++j) {
      const int er = __builtin_amdgcn_readlane(erow, j);
      float hj[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) hj[m] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, h[m]), j));
      const f32x4 e = *(const f32x4*)(emb + (size_t)er * 256 + lane * 4);
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float v = b3[k];
#pragma unroll
        for (int m = 0; m < 16; ++m) v = fmaf(w[k][m], hj[m], v);
        o[k] = e[k] + v;
      }
      const size_t at = (size_t)(q0 + j) * 256 + lane * 4;
      *(f32x4*)(keys + at) = o;
      if (keys_lp) {
        Lp4<TL> l;
#pragma unroll
        for (int k = 0; k < 4; ++k) l[k] = (TL)o[k];
        *(Lp4<TL>*)(keys_lp + at) = l;
      }
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void multimask_out_kernel(const float* __restrict__ masks, const float* __restrict__ iou, int iou_ld, float* __restrict__ low3,
                                                           float* __restrict__ iou3, long long P) {
  // grid.y = pair; tokens 1..3 of masks [n, 4, P] are 3 * P contiguous floats
  const int b = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x < 3) iou3[b * 3 + threadIdx.x] = iou[(size_t)b * iou_ld + 1 + threadIdx.x];
  const float* src = masks + ((size_t)b * 4 + 1) * P;
  float* dst = low3 + (size_t)b * 3 * P;
  const long long n = VEC ? 3 * P / 4 : 3 * P;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    if (VEC) ((f32x4*)dst)[i] = ((const f32x4*)src)[i];
    else dst[i] = src[i];
  }
}

// torch.argmax over NM values: the lowest index among equal maxima; a NaN counts as greater than every number (the first NaN wins)
template <int NM> __device__ __forceinline__ int argmax_first(const float* __restrict__ v) {
  int sel = 0;
  float best = v[0];
#pragma unroll
  for (int k = 1; k < NM; ++k) {
    const float x = v[k];
    if (best == best && (x != x || x > best)) { best = x; sel = k; }
  }
  return sel;
}

template <int NM>
__global__ __launch_bounds__(NT) void best_candidate_kernel(const float* __restrict__ low_res, const float* __restrict__ iou, float* __restrict__ mask_out,
                                                            int* __restrict__ sel_out, int P4) {
  // grid.y = pair; P4 = P / 4 16-byte groups per plane
  const int b = blockIdx.y;
  const int sel = argmax_first<NM>(iou + (size_t)b * NM);
  if (sel_out && blockIdx.x == 0 && threadIdx.x == 0) sel_out[b] = sel;
  const f32x4* src = (const f32x4*)low_res + ((size_t)b * NM + sel) * P4;
  f32x4* dst = (f32x4*)mask_out + (size_t)b * P4;
  for (int i = blockIdx.x * NT + threadIdx.x; i < P4; i += gridDim.x * NT) dst[i] = src[i];
}

constexpr int M2M_GRID_X = 64;                // workgroups per pair, as best_candidate_kernel's: M2M_GRID_X * NT 16-byte groups per pass of the loop

// torch.clamp(v, -c, c) bit for bit: comparisons, so that a NaN fails both and stays, -0.0 lies inside and stays, +-inf become +-c
__device__ __forceinline__ float clamp_keep_nan(float v, float c) { return v < -c ? -c : (v > c ? c : v); }

template <int NM>
__global__ __launch_bounds__(NT) void m2m_fanout_kernel(const float* __restrict__ low_res, float c, float* __restrict__ mask_out, const float* __restrict__ coords,
                                                        const int* __restrict__ labels, const int* __restrict__ pair_image, float* __restrict__ coords_out,
                                                        int* __restrict__ labels_out, int* __restrict__ pair_image_out, int G, int K) {
  // grid.y = pair; G = NM * P / 4 16-byte groups of the pair's NM planes, which are contiguous on both sides (candidate-major inside the pair)
  const size_t b = blockIdx.y;
  const f32x4* src = (const f32x4*)low_res + b * G;
  f32x4* dst = (f32x4*)mask_out + b * G;
  for (int i = blockIdx.x * NT + threadIdx.x; i < G; i += gridDim.x * NT) {
    const f32x4 v = src[i];
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = clamp_keep_nan(v[k], c);
    dst[i] = o;
  }
  if (blockIdx.x == 0) {                                                 // the pair's prompt rows, written NM times
    for (int t = threadIdx.x; t < NM * K * 2; t += NT) coords_out[b * NM * K * 2 + t] = coords[b * K * 2 + t % (K * 2)];
    for (int t = threadIdx.x; t < NM * K; t += NT) labels_out[b * NM * K + t] = labels[b * K + t % K];
    if (pair_image_out && threadIdx.x < NM) pair_image_out[b * NM + threadIdx.x] = pair_image[b];
  }
}

}  // namespace

// pair_image == nullptr: B * rep image-major pairs; else B pairs (rep = 1) whose images the device table names
static int mask_prompt_embed_launch(const float* mask, const float* emb, const float* params, float* keys, void* keys_lp, int lp_dtype, int B, int rep,
                                    int fs, const int* pair_image, cvmi_stream_t stream_) {
  CVMI_CHECK(mask && emb && params && keys && B > 0 && rep > 0 && fs > 0, "mask_prompt_embed: bad arguments");
  CVMI_CHECK(!keys_lp || lp_dtype == CVMI_F16 || lp_dtype == CVMI_BF16, "mask_prompt_embed: the 16-bit copy must be CVMI_F16 or CVMI_BF16");
  CVMI_CHECK((((uintptr_t)mask | (uintptr_t)emb | (uintptr_t)params | (uintptr_t)keys) & 15) == 0 && ((uintptr_t)keys_lp & 7) == 0,
             "mask_prompt_embed: pointers must be 16-byte aligned (the 16-bit copy 8-byte)");
  const long long total = (long long)B * rep * fs * fs;                  // output pixels
  CVMI_CHECK(fs <= 16384 && total < (1ll << 31) - 64, "mask_prompt_embed: %lld output pixels: the pixel count must stay below 2^31", total);
  const int grid = (int)std::min<long long>((total + NT - 1) / NT, GRID_CAP);
  hipStream_t s = (hipStream_t)stream_;
  if (keys_lp && lp_dtype == CVMI_BF16) {
    cvmi_note_kernel("mask_prompt_embed_kernel<__bf16>");
    hipLaunchKernelGGL(mask_prompt_embed_kernel<__bf16>, dim3(grid), dim3(NT), 0, s, mask, emb, params, keys, (__bf16*)keys_lp, rep, fs, (int)total, pair_image);
  } else {
    cvmi_note_kernel("mask_prompt_embed_kernel<_Float16>");
    hipLaunchKernelGGL(mask_prompt_embed_kernel<_Float16>, dim3(grid), dim3(NT), 0, s, mask, emb, params, keys, (_Float16*)keys_lp, rep, fs, (int)total, pair_image);
  }
  CVMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int cvmi_mask_prompt_embed(const float* mask, const float* emb, const float* params, float* keys, void* keys_lp, int lp_dtype, int B, int rep,
                                      int fs, cvmi_stream_t stream_) {
  return mask_prompt_embed_launch(mask, emb, params, keys, keys_lp, lp_dtype, B, rep, fs, nullptr, stream_);
}

extern "C" int cvmi_mask_prompt_embed_pairs(const float* mask, const float* emb, const float* params, float* keys, void* keys_lp, int lp_dtype, int n_pairs,
                                            const int* pair_image, int fs, cvmi_stream_t stream_) {
  CVMI_CHECK(pair_image && ((uintptr_t)pair_image & 3) == 0, "mask_prompt_embed_pairs: the pair table must be a 4-byte aligned device pointer");
  return mask_prompt_embed_launch(mask, emb, params, keys, keys_lp, lp_dtype, n_pairs, 1, fs, pair_image, stream_);
}

extern "C" int cvmi_multimask_out(const float* masks, const float* iou, int iou_ld, float* low_res3, float* iou3, int n, int P, cvmi_stream_t stream_) {
  CVMI_CHECK(masks && iou && low_res3 && iou3 && n > 0 && n <= 65535 && P > 0 && iou_ld >= 4, "multimask_out: bad arguments");
  const bool vec = P % 4 == 0 && (((uintptr_t)masks | (uintptr_t)low_res3) & 15) == 0;
  const int grid = (int)std::min<long long>((3ll * P / (vec ? 4 : 1) + NT - 1) / NT, 64);
  const dim3 g(grid, n), b(NT);
  cvmi_note_kernel(vec ? "multimask_out_kernel<true>" : "multimask_out_kernel<false>");
  if (vec) hipLaunchKernelGGL(multimask_out_kernel<true>, g, b, 0, (hipStream_t)stream_, masks, iou, iou_ld, low_res3, iou3, (long long)P);
  else hipLaunchKernelGGL(multimask_out_kernel<false>, g, b, 0, (hipStream_t)stream_, masks, iou, iou_ld, low_res3, iou3, (long long)P);
  CVMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int cvmi_best_candidate(const float* low_res, const float* iou, int NM, float* mask_out, int* sel_out, int n, int P, cvmi_stream_t stream_) {
  CVMI_CHECK(NM == 1 || NM == 3, "best_candidate: NM = %d candidates: 1 or 3", NM);
  CVMI_CHECK(n >= 0 && n <= 65535 && P > 0 && P % 4 == 0, "best_candidate: n = %d pairs of P = %d logits: n in 0 .. 65535, P a positive multiple of 4", n, P);
  if (n == 0) return 0;
  CVMI_CHECK(low_res && iou && mask_out, "best_candidate: bad arguments");
  CVMI_CHECK((((uintptr_t)low_res | (uintptr_t)iou | (uintptr_t)mask_out) & 15) == 0 && ((uintptr_t)sel_out & 3) == 0,
             "best_candidate: pointers must be 16-byte aligned (sel_out 4-byte)");
  const int P4 = P / 4;
  const dim3 g(std::min((P4 + NT - 1) / NT, 64), n), b(NT);
  hipStream_t s = (hipStream_t)stream_;
  if (NM == 3) {
    cvmi_note_kernel("best_candidate_kernel<3>");
    hipLaunchKernelGGL(best_candidate_kernel<3>, g, b, 0, s, low_res, iou, mask_out, sel_out, P4);
  } else {
    cvmi_note_kernel("best_candidate_kernel<1>");
    hipLaunchKernelGGL(best_candidate_kernel<1>, g, b, 0, s, low_res, iou, mask_out, sel_out, P4);
  }
  CVMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int cvmi_m2m_fanout(const float* low_res, int NM, float clamp, float* mask_out, const float* coords, const int* labels, const int* pair_image,
                               float* coords_out, int* labels_out, int* pair_image_out, int n, int P, int K, cvmi_stream_t stream_) {
  CVMI_CHECK(NM == 1 || NM == 3, "m2m_fanout: NM = %d candidates: 1 or 3", NM);
  CVMI_CHECK(n >= 0 && n <= 65535 && P > 0 && P % 4 == 0 && P <= (1 << 28) && K > 0 && K <= 65536,
             "m2m_fanout: n = %d pairs of P = %d logits and K = %d tokens: n in 0 .. 65535, P a positive multiple of 4 up to 2^28, K in 1 .. 65536", n, P, K);
  CVMI_CHECK(clamp >= 0.f, "m2m_fanout: the clamp bound must be a number >= 0");
  CVMI_CHECK((pair_image == nullptr) == (pair_image_out == nullptr), "m2m_fanout: pair_image and pair_image_out go together (both NULL: uniform plans)");
  if (n == 0) return 0;
  CVMI_CHECK(low_res && mask_out && coords && labels && coords_out && labels_out, "m2m_fanout: bad arguments");
  CVMI_CHECK((((uintptr_t)low_res | (uintptr_t)mask_out) & 15) == 0 &&
                 (((uintptr_t)coords | (uintptr_t)labels | (uintptr_t)pair_image | (uintptr_t)coords_out | (uintptr_t)labels_out | (uintptr_t)pair_image_out) & 3) == 0,
             "m2m_fanout: the planes must be 16-byte aligned (the prompt tables 4-byte)");
  const int G = NM * (P / 4);
  const dim3 g(std::min((G + NT - 1) / NT, M2M_GRID_X), n), b(NT);
  hipStream_t s = (hipStream_t)stream_;
  if (NM == 3) {
    cvmi_note_kernel("m2m_fanout_kernel<3>");
    hipLaunchKernelGGL(m2m_fanout_kernel<3>, g, b, 0, s, low_res, clamp, mask_out, coords, labels, pair_image, coords_out, labels_out, pair_image_out, G, K);
  } else {
    cvmi_note_kernel("m2m_fanout_kernel<1>");
    hipLaunchKernelGGL(m2m_fanout_kernel<1>, g, b, 0, s, low_res, clamp, mask_out, coords, labels, pair_image, coords_out, labels_out, pair_image_out, G, K);
  }
  CVMI_LAUNCH_CHECK();
  return 0;
}
