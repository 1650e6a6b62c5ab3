// Hiera stages 1 - 2 (C = 144 / 288), second half of a block in ONE launch, in place on the f32 residual stream:
//     x1 = x + ao . Wp^T + bp                                   (`x = shortcut + proj(attn)`)
//     x  <- x1 + fc2( GELU( fc1( LayerNorm(x1) ) ) ) + b2       (`x = x + mlp(norm2(x))`)
// Included by hiera_mlp.hip behind the pieces of hiera_mlp_kernel: the weight stream, both chunk-loop forms and the epilogue are those pieces as
// they stand; only the front end differs.  Unfused, the proj launch writes x1 and the MLP launch reads it straight back (1.2 GB per stage-1
// block at B = 16, 0.6 GB per stage-2 block) -- here x1 exists in registers only.
//
//   1. proj.  ao's row is the B operand as it lies in memory: lane (token lr, half lh) takes channels 16 s + 8 lh .. + 7 of k-step s with one
//      16-byte load.  Wp streams through the SAME two-slot LDS ring as the MLP's chunks, packed output tile by output tile (rows 32 t .. + 31,
//      natural k order, KS fragments per tile) and cut into pieces of TP = FR / KS tiles -- what fits a ring slot.  The products accumulate
//      into yacc[t], fc2's accumulator (VAR 2: the AGPR set the pipelined loop pins).
//   2. LayerNorm in the accumulator layout.  The lane holds x1 at channels 32 t + 8 g + 4 lh + e (register 4 g + e of tile t), x loaded where
//      the epilogue loads it.  Statistics over the lane's half row and its `lane ^ 32` partner (two passes, as hiera_mlp_kernel).  Registers
//      8 h .. 8 h + 7 of tile t, normalised and rounded, ARE fc1's B fragment of k-step 2 t + h -- no lane exchange -- so k index kappa of that
//      step stands for channel 32 t + 16 h + 8 ((kappa & 7) >> 2) + 4 (kappa >> 3) + (kappa & 3): W1 is packed with its columns in that order
//      (engine.PackedProjMlp; the permutation W2's packing applies to its k).  x1 is not written.
//   3. The chunk loop, with yacc entering as the proj product.  The epilogue re-reads x and stores  x + (yacc + (bp + b2)).
// Not bit-equal to the two launches it replaces (x1 = x + (proj + bp) is rounded once there; fc1 sums its k in another order): equal to within f32
// rounding ahead of the same 16-bit roundings.  Every association above is fixed in the source: replays are bit-identical.
#pragma once

namespace {

template <int C, int VAR> struct ProjCfg {
  using M = MlpCfg<C, VAR>;
  static_assert(M::SLOTS == 2, "the slot hand-over below is written for two slots");
  static constexpr int KS = M::KS, NT = M::NT;
  static constexpr int TP = M::FR / KS;                          // output tiles per piece
  static constexpr int NPP = (NT + TP - 1) / TP;                 // pieces
  static constexpr int BYTES = NT * KS * 1024;                   // the MLP chunks follow
  // The last piece sits in the slot the chunk loop fills SECOND (VAR 2: stage -1 goes to slot 1, so slot 0; otherwise chunk 0 goes to slot 0,
  // so slot 1): the loop's first unit is then issued under the last piece's MFMAs.
  static constexpr int slot(int p) { return ((VAR == 2 ? 0 : 1) + NPP - 1 - p) % 2; }
  static constexpr int tiles(int p) { return p == NPP - 1 ? NT - TP * (NPP - 1) : TP; }
  static_assert(TP >= 1 && NPP >= 2 && tiles(NPP - 1) >= 1 && TP * KS <= M::FR, "a piece fits a slot");
};

// the MFMAs of piece P: fragment f of the piece = (tile TP P + f / KS, k-step f % KS); A through the counted ring of hiera_mlp.hip's chunk-order
// loop.  VAR 2 issues them from asm so that yacc stays in AGPRs (the first k-step of a tile starts the accumulator from 0); both operands come
// from memory (LDS ring, global load), no VALU result feeds an MFMA here.
template <int C, int VAR, int P>
__device__ __forceinline__ void proj_piece(const char* buf, const u32x4 (&af)[MlpCfg<C, VAR>::KS], f32x16 (&yacc)[MlpCfg<C, VAR>::NT]) {
  using PC = ProjCfg<C, VAR>;
  constexpr int KS = PC::KS, NF = PC::tiles(P) * KS, PF = 6;
  static_assert(NF >= PF, "ring");
  u32x4 ring[PF];
  const unsigned lbase = (unsigned)(size_t)((const __attribute__((address_space(3))) char*)buf);
#pragma unroll
  for (int f = 0; f < PF; ++f) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(ring[f]) : "v"(lbase), "i"(f * 1024));
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int t = PC::TP * P + f / KS, s = f % KS;
    ring_wait(ring[f % PF], (NF - 1 - f) < (PF - 1) ? (NF - 1 - f) : (PF - 1));
    if constexpr (VAR == 2) {
      if (s == 0) asm volatile(CVMI_MFMA_ASM " %0, %1, %2, 0" : "=a"(yacc[t]) : "v"(ring[f % PF]), "v"(af[s]));
      else asm volatile(CVMI_MFMA_ASM " %0, %1, %2, %0" : "+a"(yacc[t]) : "v"(ring[f % PF]), "v"(af[s]));
    } else {
      yacc[t] = CVMI_MFMA_32X32X16(__builtin_bit_cast(f16x8, ring[f % PF]), __builtin_bit_cast(f16x8, af[s]), yacc[t], 0, 0, 0);
    }
    if (f + PF < NF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(ring[f % PF]) : "v"(lbase), "i"((f + PF) * 1024));
  }
}

template <int C, int VAR>
__global__ __launch_bounds__((MlpCfg<C, VAR>::NW * 64), (MlpCfg<C, VAR>::WPS)) void proj_mlp_kernel(float* __restrict__ x, int x_ld, const f16* __restrict__ ao, int ao_ld,
                                                                                     const char* __restrict__ wp, const float* __restrict__ bp,
                                                                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                                     const float* __restrict__ b2, long long rows,
                                                                                     float* __restrict__ stats_out, float stats_eps) {
  using Cfg = MlpCfg<C, VAR>;
  using PC = ProjCfg<C, VAR>;
  constexpr int KS = Cfg::KS, KS1 = Cfg::KS1, NT = Cfg::NT, CHB = Cfg::CHB, NW = Cfg::NW, NPP = PC::NPP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const MlpWave<C, VAR> w(smem, wp + PC::BYTES, rows);           // (its stream: the MLP chunks behind the proj pieces)
  const int lh = w.lh;
  float* const xr = x + w.row_clamped * (long long)x_ld;
  const f16* const ar = ao + w.row_clamped * (long long)ao_ld;

  // ---- 1. proj: piece p -> slot PC::slot(p), issued behind the barrier that retires the reads of piece p - 1 (that slot's)
  auto issue_proj = [&](auto pc) {
    constexpr int p = decltype(pc)::value;
    tok_issue_chunk<PC::tiles(p) * KS, NW>(wp + (size_t)p * PC::TP * KS * 1024, smem + PC::slot(p) * CHB, w.wv, w.lane);
  };
  issue_proj(std::integral_constant<int, 0>{});
  u32x4 af[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) af[s] = *reinterpret_cast<const u32x4*>(ar + 16 * s + 8 * lh);
  f32x16 yacc[NT];
  if constexpr (VAR != 2) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) yacc[t][r] = 0.f;
  }
  static_for<0, NPP>([&](auto pc) {
    constexpr int p = decltype(pc)::value;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // own DMA pieces of piece p (and ao's loads); the barrier publishes them
    __syncthreads();
    if constexpr (p + 1 < NPP) issue_proj(std::integral_constant<int, p + 1>{});
    else if constexpr (VAR == 2) w.issue_stage(-1);
    else w.issue_chunk(0);
    proj_piece<C, VAR, p>(smem + PC::slot(p) * CHB + w.lane * 16, af, yacc);
  });
  if constexpr (VAR == 2) {
    __syncthreads();                                             // every wave has read the last piece: its slot takes stage 0
    w.issue_stage(0);
    asm volatile("s_nop 15" : "+a"(yacc[NT - 1]));              // MFMA -> v_accvgpr_read wait states behind the last MFMA (the other tiles' are >= KS MFMAs back)
  }

  // ---- 2. LayerNorm of x1 = x + (yacc + bp) in the accumulator layout -> fc1's B fragments
  u32x4 xn[KS1];
  {
    // Loads are fenced into groups of LNG tiles: an address that passed through an asm statement naming the previous group's result cannot be
    // used before that result exists.  (Left alone hipcc hoists the whole row's x, bp, gamma and beta loads -- 4 x 72 registers at C = 144 --
    // over the accumulators and spills.)
    constexpr int LNG = 2;
    float v[NT][16];
    float s = 0.f;
    const float *xp = xr + 4 * lh, *pp = bp + 4 * lh;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t % LNG == 0 && t > 0) asm volatile("" : "+v"(xp), "+v"(pp) : "v"(s));
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (32 * t + 8 * g < C) {
          const int c0 = 32 * t + 8 * g;
          const f32x4 xv = *reinterpret_cast<const f32x4*>(xp + c0), pv = *reinterpret_cast<const f32x4*>(pp + c0);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[t][4 * g + e] = xv[e] + (yacc[t][4 * g + e] + pv[e]);
            s += v[t][4 * g + e];
          }
        }
    }
    s += __shfl_xor(s, 32);
    const float mean = s / (float)C;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 2 * KS; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float d = v[k >> 2][4 * (k & 3) + e] - mean; q += d * d; }
    q += __shfl_xor(q, 32);
    const float rstd = 1.0f / sqrtf(q / (float)C + eps);
    const float *gp = gamma + 4 * lh, *tp = beta + 4 * lh;
#pragma unroll
    for (int k = 0; k < KS; ++k) {                                // k-step 2 t + h: registers 8 h .. 8 h + 7 of tile t
      const int t = k >> 1, h = k & 1;
      if (k % (2 * LNG) == 0 && k > 0) asm volatile("" : "+v"(gp), "+v"(tp) : "v"(xn[k - 1]));
      const int c0 = 32 * t + 16 * h;
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(gp + c0), g1 = *reinterpret_cast<const f32x4*>(gp + c0 + 8);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(tp + c0), b1 = *reinterpret_cast<const f32x4*>(tp + c0 + 8);
      f16x8 hv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        hv[e] = (f16)((v[t][8 * h + e] - mean) * rstd * g0[e] + b0[e]);
        hv[4 + e] = (f16)((v[t][8 * h + 4 + e] - mean) * rstd * g1[e] + b1[e]);
      }
      xn[k] = __builtin_bit_cast(u32x4, hv);
    }
    xn[KS] = tok_bias_fragment(lh);
  }

  // ---- 3. the chunk loop and the epilogue of hiera_mlp_kernel.  x's and the LayerNorm parameters' loads count on vmcnt like the ring's DMA
  // instructions: everything is waited for here, so the loop's own counted wait finds its first unit landed whatever else was in flight.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  mlp_chunk_loop<C, VAR>(w, xn, yacc);
  mlp_epilogue<C, VAR, true>(w, xr, yacc, b2, bp, stats_out, stats_eps);
}

template <int C, int VAR>
int launch_proj_mlp(const cvmi_mlp_desc& d, hipStream_t s) {
  using Cfg = MlpCfg<C, VAR>;
  static hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&proj_mlp_kernel<C, VAR>), hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS);
  CVMI_HIP(attr);
  const long long per = (long long)Cfg::NW * 32;
  cvmi_note_kernel("proj_mlp_kernel<%d, %d>", C, VAR);
  hipLaunchKernelGGL((proj_mlp_kernel<C, VAR>), dim3((unsigned)((d.rows + per - 1) / per)), dim3(Cfg::NW * 64), Cfg::LDS, s, (float*)d.x, d.x_ld, (const f16*)d.ao,
                     d.ao_ld, (const char*)d.w_packed, d.bp, d.gamma, d.beta, d.eps, d.b2, d.rows, d.ln_stats_out, d.ln_stats_eps);
  CVMI_LAUNCH_CHECK();
  return 0;
}

// the proj form of cvmi_hiera_mlp (x, gamma, beta, b2, rows, C in {144, 288}, the dtype and ln_stats_out are checked by the caller)
int proj_mlp_dispatch(const cvmi_mlp_desc& d, hipStream_t s) {
  CVMI_CHECK(d.ao && d.w_packed && d.bp, "proj_mlp: needs ao, the packed weights and bp");
  CVMI_CHECK((((uintptr_t)d.ao | (uintptr_t)d.w_packed | (uintptr_t)d.bp) & 15) == 0, "proj_mlp: ao / weights / bp are not aligned to 16 bytes");
  const int C = d.C;
  CVMI_CHECK(d.ao_ld >= C && d.ao_ld % 8 == 0, "proj_mlp: ao_ld=%d must be >= C and a multiple of 8", d.ao_ld);
  if (C == 144) return launch_proj_mlp<144, 1>(d, s);
  return launch_proj_mlp<288, 2>(d, s);
}

}  // namespace
