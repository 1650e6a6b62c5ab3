// Token-stationary linear layer for the short-K GEMMs of Hiera (K = C = 144 and 288; K = 576 is tok_linear16.hip):
//     y[r, n] = act( sum_k in[r, k] * W[n, k] + b[n] )        in = LayerNorm(x[r, :]) (f32 stream, fused) or an fp16 matrix
//     out: fp16 [rows, N]   or   f32 residual stream updated in place:  res[r, n] += y[r, n]
// (sam2 hieradet MultiScaleBlock: `qkv(norm1(x))`, `x = shortcut + proj(attn)`, `mlp.layers[0](norm2(x))` + GELU; behind
//  /root/reference/src/sam2_infer.py:226.)
//
// Why not the tiled GEMM: with K = 144 .. 576 a 256 x 256 tile runs only 3 .. 9 K-steps, so its prologue, epilogue and the
// LayerNorm pass in front of it weigh as much as the MFMAs.  Here a wave keeps its 32 rows as the B fragments of the MFMA for
// the whole launch (K/16 x 4 registers) and walks the output channels 32 at a time: per chunk K/16 + 1 MFMAs (the extra k-step
// carries the bias as a hi + lo fp16 pair against constant-1 columns), A = the weight chunk in fragment order, streamed
// L2 -> LDS by global_load_lds into a ring and read lane-linearly (conflict-free ds_read_b128, kept PF deep in flight).  Only
// the A operand comes from LDS -- half the LDS traffic of a tiled GEMM -- and the accumulator of a chunk is its epilogue:
// lane = row, registers = 4 consecutive channels per group -> 8-byte fp16 / 16-byte f32 stores.
// 8 waves per workgroup, 256 rows; the two waves of a SIMD run half a chunk interval apart (ping-pong schedule, below): one in its
// MFMAs beside the other in its epilogue VALU, stores and weight prefetch.
#include "tok_stream.hpp"

namespace {

template <int K> struct TlCfg {
  static_assert(K == 144 || K == 288, "the instances that are built (K = 576: tok_linear16.hip)");
  static constexpr int KS = K / 16, KS1 = KS + 1;
  static constexpr int CHB = KS1 * 1024;                       // bytes per 32-channel weight chunk
  static constexpr int SLOTS = 4;                               // ring depth
  static constexpr int LDS = SLOTS * CHB + TL_NW * TL_STG;     // + the per-wave stage of the staged store
};

// LN = 1: `in` is the f32 stream (ld in_ld), normalised with gamma / beta / eps.  LN = 0: `in` is fp16 [rows, in_ld].  LN = 2: f32 rows
// converted as they are (the neck's lateral convs read the stage outputs of the f32 stream: no cast pass).
// RES = true: out is f32 (ld out_ld), out[r, n] += y.  RES = false: out is fp16.
template <int K, int LN, bool RES, bool GELU, bool TSTORE, bool POOL = false>
__global__ __launch_bounds__(TL_NW * 64, 2) void tok_linear_kernel(const void* __restrict__ in, int in_ld, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float eps, const char* __restrict__ wp,
                                                                   void* __restrict__ out, int out_ld, long long rows, int N, const TlExtra ex) {
  using Cfg = TlCfg<K>;
  constexpr int KS = Cfg::KS, KS1 = Cfg::KS1, CHB = Cfg::CHB, SLOTS = Cfg::SLOTS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lr = lane & 31, lh = lane >> 5;
  // rows % 256 == 0 (checked by the host): every row exists.  POOL: the lane reads the token of its 2 x 2 block (tok_stream.hpp: pool_token);
  // out is the pooled [B, H/2, W/2, N] f32 map, row prow.
  const long long wrow0 = ((long long)blockIdx.x * TL_NW + wv) * 32;
  long long row = wrow0 + lr, prow = 0;
  if constexpr (POOL) row = pool_token(row, lr, ex, prow);
  const int nch = (N + 31) / 32;

  auto issue_chunk = [&](int j) { tok_issue_chunk<KS1>(wp + (size_t)j * CHB, smem + (j % SLOTS) * CHB, wv, lane); };   // chunk j -> ring slot j % SLOTS
#pragma unroll
  for (int j = 0; j < SLOTS - 1; ++j)
    if (j < nch) issue_chunk(j);

  // ---- B fragments: lane (row lr, half lh) holds in[row][16 s + 8 lh .. + 7]
  u32x4 xn[KS1];
  if constexpr (LN == 2) {
    const float* xr = reinterpret_cast<const float*>(in) + row * (long long)in_ld;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      if (k % 3 == 0) __builtin_amdgcn_sched_barrier(0);
      const f32x4 a = *reinterpret_cast<const f32x4*>(xr + 16 * k + 8 * lh), b = *reinterpret_cast<const f32x4*>(xr + 16 * k + 8 * lh + 4);
      f16x8 h;
#pragma unroll
      for (int e = 0; e < 4; ++e) { h[e] = (f16)a[e]; h[4 + e] = (f16)b[e]; }
      xn[k] = __builtin_bit_cast(u32x4, h);
    }
  } else if constexpr (LN == 1) {
    // The statistics first (forwarded, or a pass of their own over the row: tok_stream.hpp), then one pass that writes the fp16 fragments.
    const float* xr = reinterpret_cast<const float*>(in) + row * (long long)in_ld;
    const float2 st = tok_ln_stats<K, 16, 2>(ex, row, xr, 8 * lh, eps);
    const float mean = st.x, rstd = st.y;
    tok_ln_fragments<KS>(xr, gamma, beta, mean, rstd, lh, xn);
  } else {
    const f16* xr = reinterpret_cast<const f16*>(in) + row * (long long)in_ld;
#pragma unroll
    for (int k = 0; k < KS; ++k) xn[k] = *reinterpret_cast<const u32x4*>(xr + 16 * k + 8 * lh);
  }
  xn[KS] = tok_bias_fragment(lh);                           // bias step: constant-1 columns k = K, K + 1

  // Epilogue of chunk j: lane (row lr, half lh), register group g -> channels 32 j + 8 g + 4 lh .. + 3.
  // RES: the four residual loads of chunk j - 1 are ordinary loads issued right after the barrier of interval j; their first use sits in
  // the MIDDLE of the interval's MFMA sequence.  Beside in-flight LDS-DMA hipcc answers an ordinary load's first use with vmcnt(0):
  // placed there the wait finds the loads and the interval's weight prefetch long landed, and the stores that follow have the second
  // half of the MFMAs to complete in before the next barrier's vmcnt(0).
  f32x4 r4[4];
  auto res_load = [&](int j) {
    const float* o = reinterpret_cast<const float*>(out) + row * (long long)out_ld + 32 * j + 4 * lh;
#pragma unroll
    for (int g = 0; g < 4; ++g) {                              // (the last chunk of N = 144 is half a chunk: no read past the row's end --
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};                     //  for the buffer's last row that would be a read past the allocation)
      r4[g] = 32 * j + 8 * g + 4 * lh < N ? *reinterpret_cast<const f32x4*>(o + 8 * g) : z;
    }
  };
  // 16-bit outputs leave through the wave's LDS stage as whole row pieces (TSTORE: tok_stream.hpp, stage_store) or, where N or out_ld
  // is no multiple of 8, straight from the accumulator layout as 8-byte pieces.
  ShiftedSums st;                                              // RES + stats_out: over the row's updated values (this lane's half), shift = the first of them
  char* const stage = smem + SLOTS * CHB + wv * TL_STG;
  auto epilogue = [&](const f32x16& acc, int j) {
    if constexpr (POOL) {
      // 2 x 2 max over the lane quad, then the quad's first lane stores
      float* o = reinterpret_cast<float*>(out) + prow * (long long)out_ld + 32 * j + 4 * lh;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = quad_max(acc[4 * g + e]);
        if ((lr & 3) == 0 && 32 * j + 8 * g + 4 * lh < N) *reinterpret_cast<f32x4*>(o + 8 * g) = v;
      }
    } else if constexpr (RES) {
      float* o = reinterpret_cast<float*>(out) + row * (long long)out_ld + 32 * j + 4 * lh;
      const bool stats = ex.stats_out != nullptr;              // (uniform)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 v = r4[g];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += acc[4 * g + e];
        if (stats && j == 0 && g == 0) st.shift = __shfl(v[0], lr);      // the row's first updated value (held by the lane of half 0)
        if (32 * j + 8 * g + 4 * lh < N) {
          *reinterpret_cast<f32x4*>(o + 8 * g) = v;
          if (stats) st.add(v);
        }
      }
    } else {
      f16* o = reinterpret_cast<f16*>(out) + row * (long long)out_ld + 32 * j + 4 * lh;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f16x4 h4 = tok_pack4<GELU>(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
        if constexpr (TSTORE) stage_put(stage, lr, 8 * g + 4 * lh, h4);
        else if (32 * j + 8 * g + 4 * lh < N) *reinterpret_cast<f16x4*>(o + 8 * g) = h4;
      }
      if constexpr (TSTORE) stage_store(stage, reinterpret_cast<f16*>(out), out_ld, wrow0, j, N, lane);
    }
  };

  constexpr int PF = 8;                         // ring depth
  // The K/16 + 1 MFMAs of chunk j against its ring slot: the counted A-fragment ring of tok_stream.hpp (tok_mfma_chunk)
  auto mfma_seq = [&](int j) -> f32x16 { return tok_mfma_chunk<KS1, PF>(smem + (j % SLOTS) * CHB + lane * 16, xn); };
  tok_pingpong<RES, SLOTS - 1>(wv < TL_NW / 2, 0, nch, res_load, mfma_seq, issue_chunk, epilogue,
                               [](f32x16& acc) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(acc) :: "memory"); });
  if constexpr (RES) {
    if (ex.stats_out) {                                        // after the last chunk's epilogue
      const float2 mr = shifted_mean_rstd(st.shift, row_sum<2>(st.s), row_sum<2>(st.q), (float)N, ex.stats_eps);
      if (lh == 0) *reinterpret_cast<float2*>(ex.stats_out + 2 * row) = mr;
    }
  }
}

template <int K, int LN, bool RES, bool GELU, bool TSTORE, bool POOL = false>
int launch_tl1(const cvmi_tok_desc& d, hipStream_t s, const TlExtra& ex) {
  using Cfg = TlCfg<K>;
  static hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&tok_linear_kernel<K, LN, RES, GELU, TSTORE, POOL>), hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS);
  CVMI_HIP(attr);
  cvmi_note_kernel("tok_linear_kernel<%d, %d, %s, %s, %s, %s>", K, LN, CVMI_BOOLNAME(RES), CVMI_BOOLNAME(GELU), CVMI_BOOLNAME(TSTORE), CVMI_BOOLNAME(POOL));
  hipLaunchKernelGGL((tok_linear_kernel<K, LN, RES, GELU, TSTORE, POOL>), dim3((unsigned)(d.rows / 256)), dim3(TL_NW * 64), Cfg::LDS, s, d.in, d.in_ld, d.gamma, d.beta,
                     d.eps, (const char*)d.w_packed, d.out, d.out_ld, d.rows, d.N, ex);
  CVMI_LAUNCH_CHECK();
  return 0;
}

template <int K, int LN, bool RES, bool GELU>
int launch_tl(const cvmi_tok_desc& d, hipStream_t s, const TlExtra& ex) {
  // TSTORE: chunks leave through the wave's LDS stage as whole 64-byte row pieces; the residual form and unaligned outputs store directly
  if constexpr (!RES) {
    if (d.N % 8 == 0 && d.out_ld % 8 == 0) return launch_tl1<K, LN, RES, GELU, true>(d, s, ex);
  }
  return launch_tl1<K, LN, RES, GELU, false>(d, s, ex);
}

template <int K>
int dispatch_tl(const cvmi_tok_desc& d, hipStream_t s, const TlExtra& ex) {
  const int ln = d.in_f32_layernorm, act = d.act;
  const bool res = d.out_f32_residual != 0;
  if (ln == 2) return launch_tl<K, 2, false, false>(d, s, ex);
  return tok_dispatch(ln != 0, res, act == CVMI_ACT_GELU, [&](auto LN, auto RES, auto GELU) {
    return launch_tl<K, decltype(LN)::value, decltype(RES)::value, decltype(GELU)::value>(d, s, ex);
  });
}

}  // namespace

// K = 576 is served by tok_linear16.hip (16x16x32 MFMA shape, its own packed-weight format)
int CVMI_ENTRY(cvmi_tok_linear16_launch)(const cvmi_tok_desc& d, hipStream_t s, const TlExtra& ex);
int CVMI_ENTRY(cvmi_tok_linear16_shares)(const cvmi_tok_desc& d);
static int tl_format(int K) { return K == 576 ? 16 : 32; }

#ifndef CVMI_OPERAND_BF16
extern "C" int cvmi_tok_linear_format(int K) { return tl_format(K); }
int CVMI_ENTRY(cvmi_tok_linear16_splits)(long long rows, int N);
extern "C" int cvmi_tok_linear_stats_parts(long long rows, int K, int N) {
  if (rows <= 0 || rows % 256 || N <= 0 || tl_format(K) != 16) return 0;
  const int ns = CVMI_ENTRY(cvmi_tok_linear16_splits)(rows, N);
  return ns > 1 ? ns : 0;
}

extern "C" int cvmi_tok_linear_supported(int K) { return K == 144 || K == 288 || K == 576; }

extern "C" size_t cvmi_tok_linear_packed_bytes(int K, int N) {
  if (!cvmi_tok_linear_supported(K) || N <= 0) return 0;
  if (tl_format(K) == 16) return (size_t)((N + 31) / 32) * (size_t)(K / 16 + 1) * 1024;     // 2 K/32 weight fragments + the bias piece per chunk
  return (size_t)(((N + 31) / 32 + 1) / 2 * 2) * (size_t)(K / 16 + 1) * 1024;        // chunk count padded to even
}
extern "C" int cvmi_tok_linear_bf16(const cvmi_tok_desc* d, cvmi_stream_t stream_);
#endif

namespace {

// The plain form (pool_h = pool_w = 0) of cvmi_tok_desc, checked before any launch; the field documentation is in include/cvmi355.h.
int check_tok(const cvmi_tok_desc& d) {
  const int ln = d.in_f32_layernorm;
  const bool res = d.out_f32_residual != 0;
  CVMI_CHECK(d.in && d.w_packed && d.out && d.rows > 0 && d.rows % 256 == 0 && d.N > 0, "tok_linear: bad arguments (rows must be a multiple of 256)");
  CVMI_CHECK(d.K == 144 || d.K == 288 || d.K == 576, "tok_linear: K=%d is not built (144, 288, 576)", d.K);
  CVMI_CHECK(ln != 1 || (d.gamma && d.beta), "tok_linear: LayerNorm input needs gamma / beta");
  CVMI_CHECK(ln >= 0 && ln <= 2 && (ln != 2 || (!res && d.act == CVMI_ACT_NONE)), "tok_linear: in_f32_layernorm must be 0, 1 or 2 (2: 16-bit output, no activation)");
  CVMI_CHECK(d.act == CVMI_ACT_NONE || (d.act == CVMI_ACT_GELU && !res), "tok_linear: act must be NONE, or GELU with 16-bit output");
  CVMI_CHECK((!d.ln_stats_in || ln == 1) && (!d.ln_stats_out || res) && (((uintptr_t)d.ln_stats_in | (uintptr_t)d.ln_stats_out) & 7) == 0,
             "tok_linear: ln_stats_in needs the LayerNorm input form, ln_stats_out the residual output form (8-byte aligned)");
  // The layout of ln_stats_out is the launch's to decide (row-block sharing writes per-slice pairs): the caller states the one it allocated
  const int writes = cvmi_tok_linear_stats_parts(d.rows, d.K, d.N);
  CVMI_CHECK(!d.ln_stats_out || d.ln_stats_out_parts == writes,
             "tok_linear: ln_stats_out_parts=%d, but this launch writes ln_stats_out in %d parts (cvmi_tok_linear_stats_parts)", d.ln_stats_out_parts, writes);
  // Workgroups that share a row block each normalise all of its rows and update their own channel slice of them: in place, one would read what another wrote
  if (ln == 1 && res && tl_format(d.K) == 16 && CVMI_ENTRY(cvmi_tok_linear16_shares)(d) > 1) {
    const uintptr_t in0 = (uintptr_t)d.in, out0 = (uintptr_t)d.out;
    const uintptr_t in1 = in0 + (uintptr_t)d.rows * (uintptr_t)d.in_ld * 4, out1 = out0 + (uintptr_t)d.rows * (uintptr_t)d.out_ld * 4;
    CVMI_CHECK(in1 <= out0 || out1 <= in0, "tok_linear: LayerNorm input and residual output overlap in a launch whose workgroups share row blocks");
  }
  CVMI_CHECK(d.in_ld >= d.K && d.in_ld % (ln ? 4 : 8) == 0 && d.out_ld >= d.N && d.out_ld % 4 == 0 && d.N % 4 == 0 &&
                 (((uintptr_t)d.in | (uintptr_t)d.w_packed | (uintptr_t)d.out) & 15) == 0 && (ln != 1 || (((uintptr_t)d.gamma | (uintptr_t)d.beta) & 15) == 0),
             "tok_linear: pointers / ld not aligned (in_ld=%d out_ld=%d N=%d)", d.in_ld, d.out_ld, d.N);
  CVMI_CHECK(d.ln_stats_in_parts >= 0 && d.ln_stats_in_parts <= 64, "tok_linear: ln_stats_in_parts out of range");
  CVMI_CHECK(ln != 2 || tl_format(d.K) != 16, "tok_linear: plain f32 input (in_f32_layernorm = 2) is built for K = 144 and 288");
  return 0;
}

// The pool form: out[b, y, x, :] = max over the 2 x 2 token block of ( LayerNorm(in[b, 2y + dy, 2x + dx, :]) W^T + bias ): the shortcut path of a Hiera
// q-pooling block, `do_pool(self.proj(x_norm))` (sam2 hieradet MultiScaleBlock.forward, behind /root/reference/src/sam2_infer.py:226), in one
// launch -- the full-resolution f32 projection (1.2 GB at the stage 1 -> 2 transition, B = 16) is neither written nor read back.
int check_tok_pool(const cvmi_tok_desc& d) {
  const int H = d.pool_h, W = d.pool_w;
  CVMI_CHECK(d.in && d.w_packed && d.out && d.gamma && d.beta && d.rows > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && d.rows % ((long long)H * W) == 0 &&
                 d.rows % 256 == 0 && d.N > 0,
             "tok_linear_pool: bad arguments (H, W even; B*H*W a multiple of 256)");
  CVMI_CHECK(d.in_f32_layernorm == 1 && !d.out_f32_residual && d.act == CVMI_ACT_NONE && !d.ln_stats_out && d.ln_stats_in_parts == 0,
             "tok_linear_pool: the pool form takes the LayerNorm input form and writes f32: no residual, activation, ln_stats_out or ln_stats_in_parts");
  CVMI_CHECK(d.K == 144 || d.K == 288 || d.K == 576, "tok_linear_pool: K=%d is not built (144, 288, 576)", d.K);
  CVMI_CHECK(d.in_ld >= d.K && d.in_ld % 4 == 0 && d.out_ld >= d.N && d.out_ld % 4 == 0 && d.N % 4 == 0 &&
                 (((uintptr_t)d.in | (uintptr_t)d.w_packed | (uintptr_t)d.out | (uintptr_t)d.gamma | (uintptr_t)d.beta) & 15) == 0,
             "tok_linear_pool: pointers / ld not aligned (in_ld=%d out_ld=%d N=%d)", d.in_ld, d.out_ld, d.N);
  return 0;
}

}  // namespace

extern "C" int CVMI_ENTRY(cvmi_tok_linear)(const cvmi_tok_desc* d, cvmi_stream_t stream_) {
  CVMI_CHECK(d, "tok_linear: null descriptor");
#ifndef CVMI_OPERAND_BF16
  if (d->dtype == CVMI_BF16) return cvmi_tok_linear_bf16(d, stream_);
#endif
  const bool pool = d->pool_h != 0 || d->pool_w != 0;
  CVMI_CHECK(d->dtype == CVMI_T16, pool ? "tok_linear_pool: dtype must be CVMI_F16 or CVMI_BF16" : "tok_linear: dtype must be CVMI_F16 or CVMI_BF16");
  if (const int rc = pool ? check_tok_pool(*d) : check_tok(*d)) return rc;
  hipStream_t s = (hipStream_t)stream_;
  const int K = d->K;
  const TlExtra ex{d->pool_w, (d->pool_h / 2) * (d->pool_w / 2), d->ln_stats_in, d->ln_stats_out, d->ln_stats_eps, d->ln_stats_in_parts};
  if (tl_format(K) == 16) return CVMI_ENTRY(cvmi_tok_linear16_launch)(*d, s, ex);
  if (!pool) {                                                // (first: the code object lists the kernels in the order this function names them)
    if (K == 144) return dispatch_tl<144>(*d, s, ex);
    return dispatch_tl<288>(*d, s, ex);
  }
  if (K == 144) return launch_tl1<144, 1, false, false, false, true>(*d, s, ex);
  return launch_tl1<288, 1, false, false, false, true>(*d, s, ex);
}
