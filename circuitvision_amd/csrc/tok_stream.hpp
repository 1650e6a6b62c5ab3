// The pieces that the token-stationary kernels share (tok_linear.hip: 32x32x16 MFMA, K = 144 / 288; tok_linear16.hip: 16x16x32, K = 576;
// hiera_mlp.hip: the counted ring wait and the forwarded LayerNorm statistics): a wave keeps its 32 rows as MFMA B fragments for the whole
// launch, the weights stream L2 -> LDS by global_load_lds through a ring of chunk slots, and the two waves of a SIMD run half a chunk
// interval apart.  The two MFMA shapes map lanes to (row, column piece) differently -- 2 lanes per row (lr = lane & 31, lh = lane >> 5)
// against 4 (c16 = lane & 15, g = lane >> 4) -- so every piece here takes the mapping as arguments (LPR = lanes per row, the lane's float
// offset in a row, its row) and none of them knows which kernel called it.
#pragma once
#include "common.hpp"
#include <type_traits>

constexpr int TL_NW = 8;                                       // waves per workgroup of the tok_linear kernels: 256 rows

// Optional extras of a tok_linear launch.  pool_*: the POOL form's token grid.  stats_in: LN = 1 only -- LayerNorm statistics of every row,
// written by the launch that produced the rows (the prologue then reads every row ONCE instead of twice).  stats_out: RES only -- after the
// in-place update, the (mean, rstd) over the N updated values of every row, for the LayerNorm (eps = stats_eps) of the NEXT launch.
struct TlExtra {
  int pool_w, pool_hw2;
  const float* stats_in;
  float* stats_out;
  float stats_eps;
  int stats_parts;          // 0: stats_in holds (mean, rstd) per row; P > 0: P per column slice (mean, sum of squared deviations) pairs per row
};

// ---- weight stream: the NP 1-KiB pieces of one chunk, L2 -> its ring slot; wave w moves pieces w, w + NWV, ... (NWV = waves per workgroup)
template <int NP, int NWV = TL_NW> __device__ __forceinline__ void tok_issue_chunk(const char* chunk, char* slot, int wv, int lane) {
  const char* src = chunk + lane * 16;
#pragma unroll
  for (int f = 0; f < (NP + NWV - 1) / NWV; ++f) {
    const int fi = f * NWV + wv;
    if (fi < NP)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)fi * 1024),
                                       (__attribute__((address_space(3))) void*)(slot + fi * 1024), 16, 0, 0);
  }
}

// ---- the counted wait that releases one register of a ring of in-flight ds_read_b128: at most `young` younger reads may still be
// outstanding (LDS returns data in issue order).  The count is an immediate of the instruction: `young` must fold to a constant where this
// is inlined -- the index arithmetic of a fully unrolled loop, like the offsets of the ring's reads -- or the build fails.
__device__ __forceinline__ void ring_wait(u32x4& r, int young) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(r) : "i"(young)); }

// ---- statistics of a row held by LPR lanes (2 or 4: lanes l, l ^ 32 or l, l ^ 16, l ^ 32, l ^ 48)
template <int LPR> __device__ __forceinline__ float row_sum(float x) {
#pragma unroll
  for (int m = 64 / LPR; m < 64; m *= 2) x += __shfl_xor(x, m);
  return x;
}

// Single-pass sums of (v - shift) and (v - shift)^2 over the values a lane holds.  The shift is one of the row's own values: what cancels in
// the variance is then (mean - shift)^2, bounded by the row's own spread, and the single-pass formula stays well conditioned -- unless the
// shift is the row's one outlier: (mean - shift)^2 is then up to n times the variance (hiera_mlp.hip's epilogue takes two passes for that).
struct ShiftedSums {
  float shift = 0.f, s = 0.f, q = 0.f;
  __device__ __forceinline__ void add(const f32x4& v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float dv = v[e] - shift; s += dv; q = fmaf(dv, dv, q); }
  }
};
// (mean, 1 / sqrt(var + eps)) of n values from their row-wide shifted sums
__device__ __forceinline__ float2 shifted_mean_rstd(float shift, float s, float q, float n, float eps) {
  const float dm = s / n;                                      // mean - shift
  const float var = fmaxf(q / n - dm * dm, 0.f);
  return make_float2(shift + dm, 1.0f / sqrtf(var + eps));
}

// LayerNorm (mean, rstd) of row `row` of K floats at xr, from the first source there is:
//   * the pair forwarded by the producer of these rows (ex.stats_parts == 0);
//   * P = ex.stats_parts per column slice (mean, sum of squared deviations) pairs of a tiled GEMM's epilogue or a row-block-shared launch,
//     combined as Chan et al. do (equal slice sizes n = K / P, fixed order): sum_t M2_t + n sum_t (mean_t - mean)^2.  The second term as
//     n (sum mean_t^2 - P mean^2) would be a difference of nearly equal numbers of size mean^2 whenever the row's offset is common to all
//     slices (slice means then differ by O(sigma / sqrt(n)) only) -- so it is formed from the deviations instead;
//   * its own shifted single pass: this lane sums the 8 floats at xr + STEP k + off of every k-step, LPR lanes share the row.  (A second
//     pass then re-reads the row -- from L1 / L2, touched a few hundred cycles earlier -- instead of keeping K / LPR f32 registers live.)
template <int K, int STEP, int LPR>
__device__ __forceinline__ float2 tok_ln_stats(const TlExtra& ex, long long row, const float* xr, int off, float eps) {
  if (ex.stats_in && ex.stats_parts == 0) return *reinterpret_cast<const float2*>(ex.stats_in + 2 * row);
  if (ex.stats_in) {
    float ms = 0.f, m2 = 0.f;
    for (int t = 0; t < ex.stats_parts; ++t) {
      const float2 st = *reinterpret_cast<const float2*>(ex.stats_in + (row * ex.stats_parts + t) * 2);
      ms += st.x; m2 += st.y;
    }
    const float inv_p = 1.0f / (float)ex.stats_parts;
    const float mean = ms * inv_p;
    float dev = 0.f;
    for (int t = 0; t < ex.stats_parts; ++t) {
      const float d = ex.stats_in[(row * ex.stats_parts + t) * 2] - mean;
      dev = fmaf(d, d, dev);
    }
    const float var = (m2 + ((float)K * inv_p) * dev) / (float)K;
    return make_float2(mean, 1.0f / sqrtf(fmaxf(var, 0.f) + eps));
  }
  const float x0 = xr[0];
  float s = 0.f, q = 0.f;
  constexpr int UNR = 96 / STEP;                               // 96 floats' loads of a lane in flight
#pragma unroll UNR
  for (int k = 0; k < K / STEP; ++k) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(xr + STEP * k + off), b = *reinterpret_cast<const f32x4*>(xr + STEP * k + off + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float da = a[e] - x0, db = b[e] - x0;
      s += da + db;
      q = fmaf(da, da, fmaf(db, db, q));
    }
  }
  return shifted_mean_rstd(x0, row_sum<LPR>(s), row_sum<LPR>(q), (float)K, eps);
}

// ---- B fragments of the 32x32x16 format from the f32 stream (tok_linear.hip LN = 1, qkv_attn.hpp): one pass over the row that writes
// lane (row, half lh)'s LayerNorm'd values in[row][16 s + 8 lh .. + 7] of every k-step s as 16-bit fragments.
// GROUP: k-steps whose loads may be in flight together (tok_linear.hip: 3, its register budget; qkv_attn.hpp: the whole row in one round trip).
template <int KS, int GROUP = 3> __device__ __forceinline__ void tok_ln_fragments(const float* xr, const float* gamma, const float* beta, float mean, float rstd,
                                                                                  int lh, u32x4* xn) {
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    if (k % GROUP == 0) __builtin_amdgcn_sched_barrier(0);  // at most GROUP steps' loads in flight: no hoisting of all K/16 of them
    const f32x4 a = *reinterpret_cast<const f32x4*>(xr + 16 * k + 8 * lh), b = *reinterpret_cast<const f32x4*>(xr + 16 * k + 8 * lh + 4);
    const float* gp = gamma + 16 * k + 8 * lh;
    const float* bp = beta + 16 * k + 8 * lh;
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gp), g1 = *reinterpret_cast<const f32x4*>(gp + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp), b1 = *reinterpret_cast<const f32x4*>(bp + 4);
    f16x8 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      h[e] = (f16)((a[e] - mean) * rstd * g0[e] + b0[e]);
      h[4 + e] = (f16)((b[e] - mean) * rstd * g1[e] + b1[e]);
    }
    xn[k] = __builtin_bit_cast(u32x4, h);
  }
}
// the bias k-step of that format: constant-1 columns k = K, K + 1 (the packed weights carry the bias there as a hi + lo pair)
__device__ __forceinline__ u32x4 tok_bias_fragment(int lh) { return (u32x4){lh == 0 ? CVMI_ONE16X2 : 0u, 0u, 0u, 0u}; }

// ---- the KS1 = K/16 + 1 MFMAs of one 32-channel chunk of the 32x32x16 format: buf = the lane's 16 bytes in the chunk's first 1-KiB piece.
// A-fragment ring: PF ds_read_b128 stay in flight ahead of the MFMA that consumes them.  The reads and their COUNTED waits are inline asm:
// left to hipcc the same source becomes read -> lgkmcnt(0) -> MFMA (every MFMA then waits a full LDS round trip, and the matrix pipe idles
// two thirds of the time).  LDS returns data in issue order, so before MFMA f at most min(PF - 1, KS1 - 1 - f) younger reads may still be
// outstanding; nothing else of the wave may touch LDS inside the sequence, and no run-time branch may sit between a read and its wait
// (hipcc may copy values that live across a block boundary, in-flight or not).
template <int KS1, int PF> __device__ __forceinline__ f32x16 tok_mfma_chunk(const char* buf, const u32x4* xn) {
  u32x4 ring[PF];
  const unsigned lbase = (unsigned)(size_t)((const __attribute__((address_space(3))) char*)buf);
#pragma unroll
  for (int f = 0; f < PF; ++f) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(ring[f]) : "v"(lbase), "i"(f * 1024));
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int f = 0; f < KS1; ++f) {
    ring_wait(ring[f % PF], (KS1 - 1 - f) < (PF - 1) ? (KS1 - 1 - f) : (PF - 1));
    const f16x8 a = __builtin_bit_cast(f16x8, ring[f % PF]);
    acc = CVMI_MFMA_32X32X16(a, __builtin_bit_cast(f16x8, xn[f]), acc, 0, 0, 0);
    if (f + PF < KS1) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(ring[f % PF]) : "v"(lbase), "i"((f + PF) * 1024));
  }
  return acc;
}

// ---- POOL form: rows are tokens of a [B, H, W] grid (pool_w = W, pool_hw2 = (H / 2)(W / 2)) and a lane quad holds the four tokens of one
// 2 x 2 block: `row` (a multiple of 4 plus q & 3 in every quad) -> the source token (dy, dx) = ((q >> 1) & 1, q & 1) of block prow = row / 4
__device__ __forceinline__ long long pool_token(long long row, int q, const TlExtra& ex, long long& prow) {
  prow = row >> 2;
  const long long b = prow / ex.pool_hw2;
  const int r = (int)(prow - b * ex.pool_hw2), w2 = ex.pool_w >> 1;
  const int py = r / w2, px = r - py * w2;
  return b * 4 * ex.pool_hw2 + (long long)(2 * py + ((q >> 1) & 1)) * ex.pool_w + 2 * px + (q & 1);
}
// max over the lane quad: two DPP quad permutes (lanes ^ 1, lanes ^ 2)
__device__ __forceinline__ float quad_max(float a) {
  a = fmaxf(a, __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, a), 0xB1, 0xF, 0xF, true)));   // quad_perm [1,0,3,2]
  return fmaxf(a, __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, a), 0x4E, 0xF, 0xF, true)));   // quad_perm [2,3,0,1]
}

// ---- four accumulator values -> their 16-bit quad, plain or through GELU
template <bool GELU> __device__ __forceinline__ f16x4 tok_pack4(float a0, float a1, float a2, float a3) {
  if constexpr (GELU) {
    const f16x2 lo2 = gelu_fast_pk(a0, a1), hi2 = gelu_fast_pk(a2, a3);
    return (f16x4){lo2[0], lo2[1], hi2[0], hi2[1]};
  } else {
    return (f16x4){(f16)a0, (f16)a1, (f16)a2, (f16)a3};
  }
}

// ---- staged store of a chunk's 16-bit outputs.  The accumulator has the row on the lane: written out directly, every lane of a store
// touches a different cache line.  Instead the wave's 32 rows x 32 channels (64 bytes a row) go through a wave-private LDS stage --
// stage_put, rows TL_STG_LD = 64 + 16 bytes apart -- and leave as whole 64-byte row pieces: 4 lanes per row, 16 rows per instruction.
constexpr int TL_STG_LD = 80, TL_STG = 32 * TL_STG_LD;         // bytes per row / per wave
__device__ __forceinline__ void stage_put(char* stage, int r, int ch, f16x4 h4) { *reinterpret_cast<f16x4*>(stage + r * TL_STG_LD + ch * 2) = h4; }
__device__ __forceinline__ void stage_store(const char* stage, f16* out, int out_ld, long long wrow0, int j, int N, int lane) {
  const int sr = lane >> 2, pc = lane & 3;
  const int c0 = 32 * j + pc * 8;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(stage + (16 * i + sr) * TL_STG_LD + pc * 16);
    if (c0 < N) *reinterpret_cast<u32x4*>(out + (wrow0 + 16 * i + sr) * (long long)out_ld + c0) = v;
  }
}

// ---- ping-pong schedule ----------------------------------------------------------------------------------------------------------
// The two waves of a SIMD (w and w + 4) share its matrix pipe and its VALU issue.  Under one barrier per chunk both run the same
// program in phase -- epilogue beside epilogue, MFMAs beside MFMAs -- and a timer-stamped build (r02, K = 288) showed what that costs: per
// chunk 1325 cycles in the 37 MFMAs, 1254 in epilogue + prefetch issue, and 1827 + 655 waiting (the partner's MFMAs): 5061 cycles for
// 2 x 1184 cycles of matrix work per SIMD.  Here every chunk interval has TWO barriers and the halves run half an interval apart:
//     waves 0-3 (leading):   b1 | MFMAs(j)                | b2 | prefetch, epilogue(j)     |
//     waves 4-7 (trailing):  b1 | prefetch, epilogue(j-1) | b2 | MFMAs(j)                  |
// so a SIMD always holds one wave in its matrix phase beside one in its VALU / memory phase, and the accumulator of a chunk is
// consumed by the phase right after it (no copy).  Ring invariants, SLOTS = AHEAD + 1 slots: chunk c is written to slot c % SLOTS after b1
// of interval c - AHEAD -- the last reads of chunk c - SLOTS (trailing half, second phase of interval c - SLOTS) ended before that barrier
// -- and every wave waits for its own pieces (vmcnt(0), explicit: hipcc puts no wait in front of a barrier for LDS-DMA writes) at
// the end of its NEXT matrix phase, at least one barrier before b1 of interval c.  That wait also covers the wave's epilogue stores
// and residual loads, all issued a full phase earlier.
// The phases of the chunks [j0, nch) of a workgroup (chunks j0 .. j0 + AHEAD - 1 are already issued):
//   res_load(j)       RES only: the residual values of chunk j, ordinary loads whose first use sits in the epilogue
//   mfma_seq(j)       -> the accumulator of chunk j; touches LDS through the ring slot alone
//   issue_chunk(j)    the weight DMA of chunk j
//   epilogue(acc, j)  activation, stores, statistics
//   pin(acc)          `s_waitcnt vmcnt(0)` in an asm statement that names the accumulator as "+v": the wait stays behind the MFMAs
__device__ __forceinline__ void tok_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
template <bool RES, int AHEAD, typename ResLoad, typename MfmaSeq, typename IssueChunk, typename Epilogue, typename Pin>
__device__ __forceinline__ void tok_pingpong(bool leading, int j0, int nch, ResLoad&& res_load, MfmaSeq&& mfma_seq, IssueChunk&& issue_chunk,
                                             Epilogue&& epilogue, Pin&& pin) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // chunks j0 .. j0 + AHEAD - 1 (and the prologue's loads)
  decltype(mfma_seq(0)) acc{};
  if (leading) {
#pragma unroll 1
    for (int j = j0; j < nch; ++j) {
      tok_barrier();
      if constexpr (RES) res_load(j);
      acc = mfma_seq(j);
      pin(acc);
      tok_barrier();
      if (j + AHEAD < nch) issue_chunk(j + AHEAD);
      epilogue(acc, j);
    }
  } else {
#pragma unroll 1
    for (int j = j0; j < nch; ++j) {
      tok_barrier();
      if (j + AHEAD < nch) issue_chunk(j + AHEAD);
      if (j > j0) epilogue(acc, j - 1);
      if constexpr (RES) res_load(j);
      tok_barrier();
      acc = mfma_seq(j);
      pin(acc);
    }
    epilogue(acc, nch - 1);
  }
}

// ---- host: the (LayerNorm input, residual output, GELU) -> instance decision of both formats.  launch(LN, RES, GELU) receives the
// template arguments as integral constants.  (The residual form has no activation; the arguments are validated by the entry points.)
template <typename Launch> int tok_dispatch(bool ln, bool res, bool gelu, Launch&& launch) {
  constexpr std::integral_constant<int, 0> ln0{};
  constexpr std::integral_constant<int, 1> ln1{};
  constexpr std::false_type no{};
  constexpr std::true_type yes{};
  if (res) return ln ? launch(ln1, yes, no) : launch(ln0, yes, no);
  if (ln) return gelu ? launch(ln1, no, yes) : launch(ln1, no, no);
  return gelu ? launch(ln0, no, yes) : launch(ln0, no, no);
}
