// Hiera stage 1 (K = C = 144, heads of 72, 8 x 8 windows; the plain blocks and the q-pooled 144 -> 288 transition): attn(window_partition(qkv(norm1(x)))) in ONE launch.  Included by attention.hip
// behind its head_dim-72 pieces: the attention arithmetic is those macros as they stand, the projection is tok_stream.hpp's prologue, weight
// stream and counted MFMA ring as tok_linear_kernel<144> runs them, so the launch writes bit for bit what the two launches it replaces write
// -- but the [tokens, 432] qkv tensor (906 MB at B = 16, written once and read back once; [tokens, 864] in the transition) never leaves the CU.
//
// A workgroup is 4 waves = 128 window-ordered tokens = two windows; wave w holds the 32 tokens (= queries = key rows) 32 (w & 1) .. of window
// w >> 1 as MFMA B fragments for the whole launch.  The packed weight (engine.PackedQkvAttn) is the qkv matrix with its rows permuted and
// zero-padded head by head: per head QA_CQ = 3 chunks of q_h, then QA_CKV = 5 chunks of k_h | v_h.
//   q chunks: row 8 g + 4 lh + e of chunk c is q channel 32 c + 16 (g >> 1) + 8 lh + 4 (g & 1) + e (zero rows past 72), so the accumulator
//     (lane = token, registers 4 g + e) rounds straight into the B fragments SCORE_TILE72 wants -- Q never touches LDS, columns 72..79 are 0.
//   k | v chunks: natural order; the lane rounds its 4-channel groups into row `token` of the window's unpadded 144-byte K / V images.
// One barrier per chunk (weight ring of 2 slots: chunk j + 1 is in flight while chunk j is multiplied); the barrier in front of the next head's
// first chunk also publishes the K / V images, and the wave runs the head's single 64-key tile right behind it, the next chunk's DMA in flight.
// Two workgroups per CU (57 KB of LDS each): one's prologue / tile / store phases overlap the other's projection MFMAs.
// QPOOL (4 heads, `ao` on the half-resolution grid): a lane quad holds the four tokens of one 2 x 2 block (tok_stream.hpp's pool_token pattern
// inside the window), the 2 x 2 max is taken over the quad on the ROUNDED q values as LOAD_Q_FRAGS takes it, every lane of a quad then runs the
// same pooled query (a score column is independent of its neighbours) and the quad's first lane stores it.
#pragma once
#include "tok_stream.hpp"

// the projection source of a fused launch (cvmi_attn_desc.proj_*)
struct QkvSrc {
  const float* x;           // f32 stream, row = token of the [img][grid_h][grid_w] grid
  int x_ld;
  const char* wp;           // packed, permuted qkv weight
  const float* gamma; const float* beta; float eps;
  const float* stats;       // (mean, rstd) per token, or NULL
};

constexpr int QA_CQ = 3, QA_CKV = 5, QA_CH = QA_CQ + QA_CKV;   // 32-row chunks per head: q_h padded to 96 rows, k_h | v_h to 160
constexpr int QA_NW = 4, QA_SLOTS = 2;
static_assert(QA_CH % QA_SLOTS == 0, "the ring slot of a chunk is a constant of the unrolled head");
constexpr int QA_ITEM_B = 2 * 64 * ROW72 + 64;                 // K + V image of one window (+ slack for the last rows' over-reads, zeroed)

// ---- the frame that both fused kernels (qkv_attn64_kernel below, qkv_attn16_kernel in qkv_attn16.hpp) put around their attention tile.
//      A kernel keeps what differs: its window / token / query indices, where its K / V image lies and which key row a lane writes, and the tile.

// chunk geometry of input width K: KS k16 steps of the row and one of the bias, a 1-KiB piece each
template <int K> struct QaChunk {
  static constexpr int KS = K / 16, KS1 = KS + 1, CHB = KS1 * 1024;
};
template <int K> constexpr int QA_LDS64 = QA_SLOTS * QaChunk<K>::CHB + 2 * QA_ITEM_B;
static_assert(QA_LDS64<144> == 57472, "two workgroups per CU: 2 x 57472 B of the 160 KiB");

// every wave's own LDS-DMA pieces and LDS stores have landed (explicit: hipcc puts no wait in front of a bare barrier), then the barrier
__device__ __forceinline__ void qa_sync() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  tok_barrier();
}

// weight chunk j -> ring slot j % QA_SLOTS, by the NW waves of the workgroup
template <int K, int NW> __device__ __forceinline__ void qa_issue_chunk(const QkvSrc& ps, char* smem, int j, int wvg, int lane) {
  constexpr int CHB = QaChunk<K>::CHB;
  tok_issue_chunk<QaChunk<K>::KS1, NW>(ps.wp + (size_t)j * CHB, smem + (j % QA_SLOTS) * CHB, wvg, lane);
}

// B fragments of token tk of window b: tok_linear_kernel<K, 1>'s prologue on a window-ordered row (GROUP: tok_ln_fragments' load grouping)
template <int K, int GROUP> __device__ __forceinline__ void qa_row_fragments(const AttnArgs& p, const QkvSrc& ps, int b, int tk, int lh, u32x4* xn) {
  constexpr int KS = QaChunk<K>::KS;
  const long long row = tok_off_fast(p, b, tk, 1, p.win, p.grid_h, p.grid_w, p.div_win);
  const float* xr = ps.x + row * (long long)ps.x_ld;
  const TlExtra ex{0, 0, ps.stats, nullptr, 0.f, 0};
  const float2 st = tok_ln_stats<K, 16, 2>(ex, row, xr, 8 * lh, ps.eps);
  tok_ln_fragments<KS, GROUP>(xr, ps.gamma, ps.beta, st.x, st.y, lh, xn);
  xn[KS] = tok_bias_fragment(lh);
}

// the accumulator of chunk cc of a head (lane = token, registers 4 g + e) to where the tile reads it
template <bool QPOOL> __device__ __forceinline__ void qa_scatter(int cc, const f32x16& acc, u32x4* qf, char* krow, char* vrow) {
  if (cc < QA_CQ) {
    // q chunk -> B fragments 2 cc, 2 cc + 1 of the score MFMAs (the sixth would be all padding)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      if (2 * cc + s2 < QS72) {
        const f16x4 lo = tok_pack4<false>(acc[8 * s2], acc[8 * s2 + 1], acc[8 * s2 + 2], acc[8 * s2 + 3]);
        const f16x4 hi = tok_pack4<false>(acc[8 * s2 + 4], acc[8 * s2 + 5], acc[8 * s2 + 6], acc[8 * s2 + 7]);
        f16x8 h8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        if constexpr (QPOOL) {                             // 2 x 2 max over the quad's rounded values (exact in f32)
#pragma unroll
          for (int e = 0; e < 8; ++e) h8[e] = (f16)quad_max((float)h8[e]);
        }
        qf[(2 * cc + s2) % QS72] = __builtin_bit_cast(u32x4, h8);
      }
    }
  } else {
    // k | v chunk: channels 32 (cc - QA_CQ) + 8 g + 4 lh .. + 3 of [k_h (72) | v_h (72) | padding], into the lane's 144-byte row pieces
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int ch0 = 32 * (cc - QA_CQ) + 8 * g;
      const f16x4 h4 = tok_pack4<false>(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
      if (ch0 < 72) *reinterpret_cast<f16x4*>(krow + ch0 * 2) = h4;
      else if (ch0 < 144) *reinterpret_cast<f16x4*>(vrow + (ch0 - 72) * 2) = h4;
    }
  }
}

// The heads' chunks against the row fragments xn (chunk 0 is already issued), for a kernel template <K, HEADS, QPOOL> of NW waves.  One barrier
// per chunk: behind it chunk j has landed and slot (j + 1) % 2 is read out, so chunk j + 1 goes in flight; behind a head's first barrier the
// previous head's tile ATTN_TILE(h) runs (its K / V rows are overwritten from chunk QA_CQ on: three barriers away).  TAIL_BARRIER: the last tile
// reads K / V rows that other waves stored.  Reads ps, smem, wvg, lane, xn, qf, krow, vrow; its own names are hh, cc, j, acc.
// A macro on purpose: as a function template that takes the tile as a callable, hipcc inlines the tile into the loop before the loop into the
// kernel and all four instances come out with other scalar code (profiles/qkv_attn_refactor_ab.md); pasted in, they are the kernels they were.
#define QA_HEAD_LOOP(NW, TAIL_BARRIER, ATTN_TILE)                                                                                          \
  _Pragma("unroll 1") for (int hh = 0; hh < HEADS; ++hh) {                                                                                 \
    _Pragma("unroll") for (int cc = 0; cc < QA_CH; ++cc) {                                                                                 \
      const int j = hh * QA_CH + cc;                                                                                                       \
      qa_sync();                                                                                                                           \
      if (j + 1 < HEADS * QA_CH) qa_issue_chunk<K, NW>(ps, smem, j + 1, wvg, lane);                                                        \
      if (cc == 0 && hh > 0) ATTN_TILE(hh - 1);                                                                                            \
      asm volatile("" ::: "memory");                                                                                                       \
      const f32x16 acc = tok_mfma_chunk<QaChunk<K>::KS1, 8>(smem + (j % QA_SLOTS) * QaChunk<K>::CHB + lane * 16, xn);                      \
      asm volatile("" ::: "memory");                                                                                                       \
      qa_scatter<QPOOL>(cc, acc, qf, krow, vrow);                                                                                          \
    }                                                                                                                                      \
  }                                                                                                                                        \
  if constexpr (TAIL_BARRIER) qa_sync();                                                                                                   \
  ATTN_TILE(HEADS - 1)

// ---- stage 1: 8 x 8 windows, K = 144
template <int K, int HEADS, bool QPOOL>
__global__ __launch_bounds__(QA_NW * 64, 2) void qkv_attn64_kernel(const AttnArgs p, const QkvSrc ps) {
  static_assert(K == 144, "the instances that are built");
  constexpr int KS1 = QaChunk<K>::KS1, CHB = QaChunk<K>::CHB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wvg = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int sub = wvg >> 1, wv = wvg & 1;                   // window within the workgroup, wave within the window
  const int lr = lane & 31, lh = lane >> 5;
  char* const Ks = smem + QA_SLOTS * CHB + sub * QA_ITEM_B;
  char* const Vs = Ks + 64 * ROW72;
  const int b = (int)blockIdx.x * 2 + sub;                  // the window (p.B is even: checked by the host)
  // tk: this lane's token of the window, whose row it projects and whose key / value row it writes; qi: its query.  QPOOL: quad lr >> 2 is 2 x 2
  // block pb of the window's 4 x 4 blocks = pooled query pb, lane lr & 3 its token (dy, dx).
  const int pb = wv * 8 + (lr >> 2);
  const int tk = QPOOL ? (2 * (pb >> 2) + ((lr >> 1) & 1)) * 8 + 2 * (pb & 3) + (lr & 1) : wv * 32 + lr;
  const int qi = QPOOL ? pb : tk;

  qa_issue_chunk<K, QA_NW>(ps, smem, 0, wvg, lane);
  if (tid < 32) *reinterpret_cast<unsigned*>(smem + QA_SLOTS * CHB + (tid >> 4) * QA_ITEM_B + 2 * 64 * ROW72 + (tid & 15) * 4) = 0u;   // the slack behind both V images
  u32x4 xn[KS1];
  qa_row_fragments<K, QaChunk<K>::KS>(p, ps, b, tk, lh, xn);

  const float c = p.scale * 1.44269504088896340736f;
  const int li = lane & 15;
  const char* const vt = Vs + (lh + 4 * (li >> 2)) * ROW72 + (16 * (lr >> 4) + 4 * (li & 3)) * 2;      // key rows 4 apart: see key_perm72
  const char* const kq = Ks + key_perm72(lr) * ROW72 + lh * 16;
  char* const krow = Ks + tk * ROW72 + lh * 8;              // the lane's 4-channel groups of its key / value row
  char* const vrow = Vs + tk * ROW72 + lh * 8;
  u32x4 qf[QS72];

  // the single 64-key tile of head h on the wave's 32 queries, as attn_res64_kernel runs it
  auto attn_tile = [&](int h) {
    f32x16 oacc[DT72];
#pragma unroll
    for (int t = 0; t < DT72; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[t][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    SCORE_TILE72(sacc, kq + (u * 32) * ROW72 + s * 32)
    const float mx = tile_max(sacc);
    f16x8 pf[2][2];
    u32x4 p8[2];                                            // (unused: SOFTMAX_UPDATE72 names it in its discarded e4m3 branch)
    SOFTMAX_UPDATE72(P16_SUM_VALU)
    PV16_STEP(vt + (u * 32 + s * 16) * ROW72 + t * 64)
    if (!QPOOL || (lr & 3) == 0) NORMALISE_STORE(DT72, true)
  };

  // the barrier in front of a head's first chunk also publishes the K / V images of the head before it, and one more the last head's
  QA_HEAD_LOOP(QA_NW, true, attn_tile);
}

// one instance's launch.  KERN: the kernel, LDS: its dynamic LDS bytes, NW: its waves, WPW: windows per workgroup; tag: cvmi_last_kernel()'s format of (K, heads, q-pooled)
template <auto KERN, int LDS, int NW, int WPW>
int qa_launch(const char* tag, int K, int heads, bool qpool, const AttnArgs& a, const QkvSrc& ps, hipStream_t stream) {
  static hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  CVMI_HIP(attr);
  cvmi_note_kernel(tag, K, heads, CVMI_BOOLNAME(qpool));
  hipLaunchKernelGGL(KERN, dim3((unsigned)(a.B / WPW)), dim3(NW * 64), LDS, stream, a, ps);
  CVMI_LAUNCH_CHECK();
  return 0;
}

template <int K, int HEADS, bool QPOOL>
int launch_qkv_attn(const AttnArgs& a, const QkvSrc& ps, hipStream_t stream) {
  return qa_launch<&qkv_attn64_kernel<K, HEADS, QPOOL>, QA_LDS64<K>, QA_NW, 2>("qkv_attn64_kernel<%d, %d, %s>", K, HEADS, QPOOL, a, ps, stream);
}

// What both dispatchers refuse, and the projection source of what they accept.  win: the window side, K: the input width, heads / heads_pool: the
// head counts that are built (plain / q-pooled), wpw: windows per workgroup, pre: the messages' prefix.
static int qa_check(const cvmi_attn_desc* d, const AttnArgs& a, int win, int K, int heads, int heads_pool, int wpw, const char* pre, QkvSrc& ps) {
  CVMI_CHECK(d->dtype == CVMI_T16, "%s: needs a 16-bit dtype", pre);
  CVMI_CHECK(d->win == win && d->Nk == win * win && d->dqk == 72 && d->dv == 72, "%s: built for %d x %d windows of head_dim 72 (win=%d Nk=%d dqk=%d dv=%d)", pre, win, win,
             d->win, d->Nk, d->dqk, d->dv);
  CVMI_CHECK(d->proj_K == K, "%s: K=%d is not built (%d)", pre, d->proj_K, K);
  CVMI_CHECK(d->heads == (d->q_pool ? heads_pool : heads), "%s: heads=%d is not built (plain: %d heads of 72, q_pool: %d)", pre, d->heads, heads, heads_pool);
  CVMI_CHECK(d->B % wpw == 0, "%s: B=%d windows are no whole number of 128-token workgroups", pre, d->B);
  CVMI_CHECK(a.q_bdiv == 1 && a.kv_bdiv == 1 && !a.q_bmap && !a.kv_bmap, "%s: no batch sharing", pre);
  CVMI_CHECK(d->proj_w && d->proj_gamma && d->proj_beta, "%s: needs the packed weight and gamma / beta", pre);
  CVMI_CHECK(d->proj_ld >= d->proj_K && d->proj_ld % 4 == 0 &&
                 (((uintptr_t)d->proj_x | (uintptr_t)d->proj_w | (uintptr_t)d->proj_gamma | (uintptr_t)d->proj_beta) & 15) == 0 && ((uintptr_t)d->proj_stats & 7) == 0,
             "%s: projection pointers / ld not aligned (proj_ld=%d)", pre, d->proj_ld);
  CVMI_CHECK(d->o_sb % 4 == 0 && d->o_sh % 4 == 0 && d->o_st % 4 == 0 && ((uintptr_t)d->o & 7) == 0, "%s: output strides must be multiples of 4 elements", pre);
  ps = QkvSrc{(const float*)d->proj_x, d->proj_ld, (const char*)d->proj_w, d->proj_gamma, d->proj_beta, d->proj_eps, d->proj_stats};
  return 0;
}

// cvmi_attention with a projection source (cvmi_attn_desc.proj_x): the shapes the fused kernel is built for, everything else refused
static int qkv_attn_dispatch(const cvmi_attn_desc* d, const AttnArgs& a, hipStream_t stream) {
  QkvSrc ps;
  if (qa_check(d, a, 8, 144, 2, 4, 2, "attention(qkv fused)", ps)) return 1;
  if (d->q_pool) return launch_qkv_attn<144, 4, true>(a, ps, stream);
  return launch_qkv_attn<144, 2, false>(a, ps, stream);
}
