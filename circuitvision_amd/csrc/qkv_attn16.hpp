// Hiera stage 2 (K = C = 288, heads of 72, 4 x 4 windows; the plain blocks and the q-pooled 288 -> 576 transition): attn(window_partition(qkv(norm1(x))))
// in ONE launch.  Included by attention.hip behind qkv_attn.hpp, whose frame it shares: QkvSrc, the head-by-head chunk order (QA_CQ q chunks, QA_CKV
// k | v chunks, engine.qkv_attn_rows -- the packed weight is engine.PackedQkvAttn of the block's qkv matrix), the chunk geometry QaChunk, the 2-slot
// weight ring (qa_issue_chunk, qa_sync), the row prologue qa_row_fragments, the accumulator scatter qa_scatter, the head / chunk loop QA_HEAD_LOOP,
// the launcher qa_launch and the host checks qa_check.  What is here is what differs: the indices, the wave-private K / V image and the tile.
// The projection is tok_stream.hpp's prologue, weight stream and counted MFMA ring as tok_linear_kernel<288, 1> runs them, so the
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
template <int K> constexpr int QW_LDS = QA_SLOTS * QaChunk<K>::CHB + QW_NW * QW_IMG_B;
static_assert(QW_LDS<288> == 76032, "two workgroups per CU: 2 x 76032 B of the 160 KiB");

template <int K, int HEADS, bool QPOOL>
__global__ __launch_bounds__(QW_NW * 64, 2) void qkv_attn16_kernel(const AttnArgs p, const QkvSrc ps) {
  static_assert(K == 288, "the instances that are built");
  constexpr int KS1 = QaChunk<K>::KS1, CHB = QaChunk<K>::CHB;
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

  qa_issue_chunk<K, QW_NW>(ps, smem, 0, wvg, lane);
  if (lane < 16) *reinterpret_cast<unsigned*>(Vs + 32 * ROW72 + lane * 4) = 0u;      // the slack behind the wave's V image
  u32x4 xn[KS1];
  qa_row_fragments<K, 6>(p, ps, b, tk, lh, xn);

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

  // every tile reads K / V rows that are the wave's own stores: no barrier in front of the last one
  QA_HEAD_LOOP(QW_NW, false, attn_tile);
}

template <int K, int HEADS, bool QPOOL>
int launch_qkv_attn16(const AttnArgs& a, const QkvSrc& ps, hipStream_t stream) {
  return qa_launch<&qkv_attn16_kernel<K, HEADS, QPOOL>, QW_LDS<K>, QW_NW, 2 * QW_NW>("qkv_attn16_kernel<%d, %d, %s>", K, HEADS, QPOOL, a, ps, stream);
}

// cvmi_attention with a projection source (cvmi_attn_desc.proj_x), win == 4 and proj_K == 288: the shapes this kernel is built for, everything else refused
static int qkv_attn16_dispatch(const cvmi_attn_desc* d, const AttnArgs& a, hipStream_t stream) {
  CVMI_CHECK(!d->av_fp8, "attention(qkv fused, 4 x 4): no fp8 AV product (av_fp8)");
  QkvSrc ps;
  if (qa_check(d, a, 4, 288, 4, 8, 2 * QW_NW, "attention(qkv fused, 4 x 4)", ps)) return 1;
  if (d->q_pool) return launch_qkv_attn16<288, 8, true>(a, ps, stream);
  return launch_qkv_attn16<288, 4, false>(a, ps, stream);
}
