// Hiera stage 2 (K = C = 288, heads of 72, 4 x 4 windows; the plain blocks and the q-pooled 288 -> 576 transition): attn(window_partition(qkv(norm1(x))))
// in ONE launch.  Included by attention.hip behind qkv_attn.hpp, whose pieces it reuses as they stand: QkvSrc, the head-by-head chunk order (QA_CQ q
// chunks, QA_CKV k | v chunks, engine.qkv_attn_rows -- the packed weight is engine.PackedQkvAttn of the block's qkv matrix), the 2-slot weight ring
// and qa_sync.  The projection is tok_stream.hpp's prologue, weight stream and counted MFMA ring as tok_linear_kernel<288, 1> runs them, so the
// rounded q, k, v are bit for bit what that launch writes into the [tokens, 864] qkv tensor (453 MB at B = 16, written once and read back once;
// [tokens, 1728] in the transition) -- which here never leaves the CU.
//
// A workgroup is 4 waves = 128 window-ordered tokens = eight windows; wave w holds the 32 tokens of windows 2 w, 2 w + 1 as MFMA B fragments for
// the whole launch (lane lr: window lr >> 4).  They are both its queries and its keys, so the K / V image (unpadded 144-byte rows, row = lr) is
// PRIVATE to the wave: no barrier publishes it, LDS serves a wave's accesses in order and the waits are the compiler's.
// The attention replaces attn_win16_kernel's per-thread dot products by the matrix pipe: per head ONE 32-key x 32-query S^T tile (5 MFMAs, the
// layout of SCORE_TILE72 with a single key half: Q from the accumulator as B fragments, score row i = key key_perm72(i)), whose registers
// 0..7 are the keys of the wave's first window and 8..15 those of the second (key_perm72(8 g + 4 lh + e) = 16 (g >> 1) + ..).  A lane takes the
// maximum, the exponentials and the sum over the 8 registers of ITS window only (the other half of the row is on lane ^ 32); P of the other
// window is zero, and as k16 step s of O^T += V^T P^T is exactly window s, the PV product (6 MFMAs, the transposing reads of PV16_STEP) is
// block-diagonal.  11 MFMAs per head and wave beside the 152 of the head's projection.
// Two workgroups per CU (74 KB of LDS each): one's prologue / tile / store phases overlap the other's projection MFMAs.
// QPOOL (8 heads, `ao` on the half-resolution grid): a lane quad holds the four tokens of one 2 x 2 block of its window, the 2 x 2 max is taken
// over the quad on the ROUNDED q values as LOAD_Q_FRAGS takes it, every lane of a quad runs the same pooled query and the quad's first lane stores.
#pragma once
#include "qkv_attn.hpp"

constexpr int QW_NW = 4;
constexpr int QW_IMG_B = 2 * 32 * ROW72 + 64;                  // K + V image of one wave's two windows (+ slack for the last rows' over-reads, zeroed)
template <int K> struct QwCfg {
  static constexpr int KS = K / 16, KS1 = KS + 1, CHB = KS1 * 1024;
  static constexpr int LDS = QA_SLOTS * CHB + QW_NW * QW_IMG_B;
};

template <int K, int HEADS, bool QPOOL>
__global__ __launch_bounds__(QW_NW * 64, 2) void qkv_attn16_kernel(const AttnArgs p, const QkvSrc ps) {
  static_assert(K == 288, "the instances that are built");
  using Cfg = QwCfg<K>;
  constexpr int KS = Cfg::KS, KS1 = Cfg::KS1, CHB = Cfg::CHB, PF = 8, NCH = HEADS * QA_CH;
  static_assert(QA_CH % QA_SLOTS == 0, "the ring slot of a chunk is a constant of the unrolled head");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wvg = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lr = lane & 31, lh = lane >> 5;
  char* const Ks = smem + QA_SLOTS * CHB + wvg * QW_IMG_B;    // the wave's own image: key row = lr
  char* const Vs = Ks + 32 * ROW72;
  const int wsel = lr >> 4;                                 // the lane's window of the wave's two
  const int b = ((int)blockIdx.x * QW_NW + wvg) * 2 + wsel;  // the window (p.B is a multiple of 8: checked by the host)
  // tk: this lane's token of the window, whose row it projects and whose key / value row (lr) it writes; qi: its query.  QPOOL: quad (lr >> 2) & 3
  // is 2 x 2 block pb of the window's 2 x 2 blocks = pooled query pb, lane lr & 3 its token (dy, dx).
  const int pb = (lr >> 2) & 3;
  const int tk = QPOOL ? (2 * (pb >> 1) + ((lr >> 1) & 1)) * 4 + 2 * (pb & 1) + (lr & 1) : lr & 15;
  const int qi = QPOOL ? pb : tk;

  auto issue_chunk = [&](int j) { tok_issue_chunk<KS1, QW_NW>(ps.wp + (size_t)j * CHB, smem + (j % QA_SLOTS) * CHB, wvg, lane); };
  issue_chunk(0);
  if (lane < 16) *reinterpret_cast<unsigned*>(Vs + 32 * ROW72 + lane * 4) = 0u;      // the slack behind the wave's V image

  // ---- B fragments of the lane's token: tok_linear_kernel<288, 1>'s prologue on a window-ordered row
  const long long row = tok_off_fast(p, b, tk, 1, p.win, p.grid_h, p.grid_w, p.div_win);
  const float* xr = ps.x + row * (long long)ps.x_ld;
  const TlExtra ex{0, 0, ps.stats, nullptr, 0.f, 0};
  const float2 st = tok_ln_stats<K, 16, 2>(ex, row, xr, 8 * lh, ps.eps);
  u32x4 xn[KS1];
  tok_ln_fragments<KS, 6>(xr, ps.gamma, ps.beta, st.x, st.y, lh, xn);
  xn[KS] = tok_bias_fragment(lh);

  const float c = p.scale * 1.44269504088896340736f;
  const int li = lane & 15;
  const char* const vt = Vs + (lh + 4 * (li >> 2)) * ROW72 + (16 * (lr >> 4) + 4 * (li & 3)) * 2;      // key rows 4 apart: see key_perm72
  const char* const kq = Ks + key_perm72(lr) * ROW72 + lh * 16;
  char* const krow = Ks + lr * ROW72 + lh * 8;              // the lane's 4-channel groups of its key / value row
  char* const vrow = Vs + lr * ROW72 + lh * 8;
  u32x4 qf[QS72];

  // the single 32-key tile of head h: the wave's two windows against themselves
  auto attn_tile = [&](int h) {
    f32x16 oacc[DT72];
#pragma unroll
    for (int t = 0; t < DT72; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[t][r] = 0.f;
    f32x16 sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < QS72; ++s) {                        // (the fifth step's reads past column 72 fetch the next row's finite data against zero Q columns)
      const f16x8 kf = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(kq + s * 32));
      sacc = CVMI_MFMA_32X32X16(kf, __builtin_bit_cast(f16x8, qf[s]), sacc, 0, 0, 0);
    }
    // the scores of the lane's own window: the other window's are masked by never being exponentiated
    float sw[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) sw[r] = wsel ? sacc[8 + r] : sacc[r];
    const float mx = max3f(max3f(sw[0], sw[1], sw[2]), max3f(sw[3], sw[4], sw[5]), fmaxf(sw[6], sw[7]));
    const float mc = xhalf_max(mx) * c;
    float psum = 0.f;
    f16x8 pw;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const float pv = __builtin_amdgcn_exp2f(fmaf(sw[r], c, -mc));
      psum += pv;
      pw[r] = (f16)pv;
    }
    const float l_run = xhalf_sum(psum);
    const u32x4 pwb = __builtin_bit_cast(u32x4, pw), zero = {0u, 0u, 0u, 0u};
    const u32x4 pf[2] = {wsel ? zero : pwb, wsel ? pwb : zero};      // P^T of k16 step s = window s
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int t = 0; t < DT72; ++t) {                      // (t = 2 reads past column 72: the next row's finite data into output rows that are never stored)
        const char* a0 = vt + (s * 16) * ROW72 + t * 64;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0 + 2 * ROW72));
        const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
        const u32x4 vv = {l2[0], l2[1], h2[0], h2[1]};
        oacc[t] = CVMI_MFMA_32X32X16(__builtin_bit_cast(f16x8, vv), __builtin_bit_cast(f16x8, pf[s]), oacc[t], 0, 0, 0);
      }
    if (!QPOOL || (lr & 3) == 0) NORMALISE_STORE(DT72, true)
  };

#pragma unroll 1
  for (int hh = 0; hh < HEADS; ++hh) {
#pragma unroll
    for (int cc = 0; cc < QA_CH; ++cc) {
      const int j = hh * QA_CH + cc;
      qa_sync();                                            // chunk j has landed; slot (j + 1) % 2 is read out
      if (j + 1 < NCH) issue_chunk(j + 1);
      if (cc == 0 && hh > 0) attn_tile(hh - 1);             // (behind the barrier: the next chunk's DMA is in flight; its K / V rows are overwritten from chunk QA_CQ on)
      asm volatile("" ::: "memory");
      const f32x16 acc = tok_mfma_chunk<KS1, PF>(smem + (j % QA_SLOTS) * CHB + lane * 16, xn);
      asm volatile("" ::: "memory");
      if (cc < QA_CQ) {
        // q chunk -> B fragments 2 cc, 2 cc + 1 of the score MFMAs (the sixth would be all padding)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          if (2 * cc + s2 < QS72) {
            const f16x4 lo = tok_pack4<false>(acc[8 * s2], acc[8 * s2 + 1], acc[8 * s2 + 2], acc[8 * s2 + 3]);
            const f16x4 hi = tok_pack4<false>(acc[8 * s2 + 4], acc[8 * s2 + 5], acc[8 * s2 + 6], acc[8 * s2 + 7]);
            f16x8 h8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            if constexpr (QPOOL) {                         // 2 x 2 max over the quad's rounded values (exact in f32)
#pragma unroll
              for (int e = 0; e < 8; ++e) h8[e] = (f16)quad_max((float)h8[e]);
            }
            qf[(2 * cc + s2) % QS72] = __builtin_bit_cast(u32x4, h8);
          }
        }
      } else {
        // k | v chunk: channels 32 (cc - QA_CQ) + 8 g + 4 lh .. + 3 of [k_h (72) | v_h (72) | padding]
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ch0 = 32 * (cc - QA_CQ) + 8 * g;
          const f16x4 h4 = tok_pack4<false>(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
          if (ch0 < 72) *reinterpret_cast<f16x4*>(krow + ch0 * 2) = h4;
          else if (ch0 < 144) *reinterpret_cast<f16x4*>(vrow + (ch0 - 72) * 2) = h4;
        }
      }
    }
  }
  attn_tile(HEADS - 1);                                     // (its K / V rows are the wave's own stores: no barrier)
}

template <int K, int HEADS, bool QPOOL>
int launch_qkv_attn16(const AttnArgs& a, const QkvSrc& ps, hipStream_t stream) {
  using Cfg = QwCfg<K>;
  static hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&qkv_attn16_kernel<K, HEADS, QPOOL>), hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS);
  CVMI_HIP(attr);
  cvmi_note_kernel("qkv_attn16_kernel<%d, %d, %s>", K, HEADS, CVMI_BOOLNAME(QPOOL));
  hipLaunchKernelGGL((qkv_attn16_kernel<K, HEADS, QPOOL>), dim3((unsigned)(a.B / (2 * QW_NW))), dim3(QW_NW * 64), Cfg::LDS, stream, a, ps);
  CVMI_LAUNCH_CHECK();
  return 0;
}

// cvmi_attention with a projection source (cvmi_attn_desc.proj_x), win == 4 and proj_K == 288: the shapes this kernel is built for, everything else refused
static int qkv_attn16_dispatch(const cvmi_attn_desc* d, const AttnArgs& a, hipStream_t stream) {
  CVMI_CHECK(d->dtype == CVMI_T16, "attention(qkv fused, 4 x 4): needs a 16-bit dtype");
  CVMI_CHECK(d->win == 4 && d->Nk == 16 && d->dqk == 72 && d->dv == 72, "attention(qkv fused, 4 x 4): built for 4 x 4 windows of head_dim 72 (win=%d Nk=%d dqk=%d dv=%d)",
             d->win, d->Nk, d->dqk, d->dv);
  CVMI_CHECK(d->proj_K == 288, "attention(qkv fused, 4 x 4): K=%d is not built (288)", d->proj_K);
  CVMI_CHECK(!d->av_fp8, "attention(qkv fused, 4 x 4): no fp8 AV product (av_fp8)");
  CVMI_CHECK(d->heads == (d->q_pool ? 8 : 4), "attention(qkv fused, 4 x 4): heads=%d is not built (plain: 4 heads of 72, q_pool: 8)", d->heads);
  CVMI_CHECK(d->B % (2 * QW_NW) == 0, "attention(qkv fused, 4 x 4): B=%d windows are no whole number of 128-token workgroups", d->B);
  CVMI_CHECK(a.q_bdiv == 1 && a.kv_bdiv == 1 && !a.q_bmap && !a.kv_bmap, "attention(qkv fused, 4 x 4): no batch sharing");
  CVMI_CHECK(d->proj_w && d->proj_gamma && d->proj_beta, "attention(qkv fused, 4 x 4): needs the packed weight and gamma / beta");
  CVMI_CHECK(d->proj_ld >= d->proj_K && d->proj_ld % 4 == 0 &&
                 (((uintptr_t)d->proj_x | (uintptr_t)d->proj_w | (uintptr_t)d->proj_gamma | (uintptr_t)d->proj_beta) & 15) == 0 && ((uintptr_t)d->proj_stats & 7) == 0,
             "attention(qkv fused, 4 x 4): projection pointers / ld not aligned (proj_ld=%d)", d->proj_ld);
  CVMI_CHECK(d->o_sb % 4 == 0 && d->o_sh % 4 == 0 && d->o_st % 4 == 0 && ((uintptr_t)d->o & 7) == 0, "attention(qkv fused, 4 x 4): output strides must be multiples of 4 elements");
  const QkvSrc ps{(const float*)d->proj_x, d->proj_ld, (const char*)d->proj_w, d->proj_gamma, d->proj_beta, d->proj_eps, d->proj_stats};
  if (d->q_pool) return launch_qkv_attn16<288, 8, true>(a, ps, stream);
  return launch_qkv_attn16<288, 4, false>(a, ps, stream);
}
