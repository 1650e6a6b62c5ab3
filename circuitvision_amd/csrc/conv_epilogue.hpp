// The LDS-transposing epilogue of the conv / GEMM kernels (igemm.hip: gemm_epilogue, gemm256_kernel, gemm256x192_kernel;
// conv_tile.hip: conv_tile_kernel, which shares the contract, Mma and tile_put4 and keeps its own store loop), each piece defined once.
//
// Rounding contract (TO = output type, act2 = act when act_after_res is set and the identity otherwise, in which case act
// has moved to act2):
//     t = TO(act(acc + bias))                 in registers, written to the LDS tile in the output type
//     y = TO(act2(float(t) + res))            when there is a residual or act_after_res; y = t otherwise
// so a 16-bit output with a residual is rounded TWICE.  The "put" loops (accumulator layout -> tile_put4) stay in the
// kernels; what follows the barrier -- residual row, residual prefetch, finishing a 16-byte chunk, storing it -- is here.
#pragma once
#include "common.hpp"

template <typename T> struct Mma;
template <> struct Mma<f16> {
  __device__ static __forceinline__ void run(const u32x4& a, const u32x4& b, f32x16& c) { mma16(a, b, c); }
};
template <> struct Mma<float> {
  __device__ static __forceinline__ void run(const u32x4& a, const u32x4& b, f32x16& c) {
    const f32x4 fa = __builtin_bit_cast(f32x4, a), fb = __builtin_bit_cast(f32x4, b);
#pragma unroll
    for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e], fb[e], c, 0, 0, 0);
  }
};

// four consecutive channels of one pixel -> their place in an epilogue's LDS tile, in the output type
template <typename TO>
__device__ __forceinline__ void tile_put4(char* d, const float (&v)[4]) {
  if constexpr (sizeof(TO) == 2) {
    f16x4 hv = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
    *reinterpret_cast<f16x4*>(d) = hv;
  } else {
    f32x4 fv = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(d) = fv;
  }
}

// residual row of output row m: plain, a constant broadcast over the batch (res_mod rows, m % res_mod), or one image's rows
// shared by res_rep consecutive batch entries (res_mod rows per image: entry e reads image e / res_rep) or by the entries a table names
// (res_map, uniform over the launch: entry e reads image res_map[e]; the host has excluded res_rep > 1 beside it)
__device__ __forceinline__ size_t res_row(int m, int res_mod, int res_rep, const int* res_map = nullptr) {
  if (res_mod <= 0) return (size_t)m;
  const int r = m % res_mod;
  if (res_map) return (size_t)res_map[m / res_mod] * (size_t)res_mod + (size_t)r;
  if (res_rep <= 1) return (size_t)r;
  return (size_t)(m / res_mod / res_rep) * (size_t)res_mod + (size_t)r;
}

// The residual of one 16-byte chunk, as finish_chunk / store_out_chunk take it: loaded where it is needed (ResLoad; base == nullptr:
// there is none) or already in a register (ResHeld, filled by RES_PREFETCH).
template <typename TO> struct ResLoad {
  const char* base; int ld; size_t row; int col;    // the chunk starts at element row * ld + col
  __device__ __forceinline__ bool has() const { return base != nullptr; }
  __device__ __forceinline__ const TO* ptr() const { return reinterpret_cast<const TO*>(base + (row * ld + col) * (int)sizeof(TO)); }
  __device__ __forceinline__ u32x4 chunk() const { return *reinterpret_cast<const u32x4*>(ptr()); }
};
struct ResHeld {
  const u32x4& v;
  __device__ __forceinline__ bool has() const { return true; }
  __device__ __forceinline__ u32x4 chunk() const { return v; }
};

// Residual prefetch into u32x4 rv[NIT]: a tile of rows m0.. and NCH chunks of type TO per row from column n0 is walked by NT threads,
// NIT chunks each (chunk tid + it * NT, row-major); rows past M read row M - 1.  Issued before the transposition, so the latency
// overlaps it instead of being paid per store-loop iteration (the compiler cannot hoist the loads over the stores: res and y may
// alias).  A macro on purpose: hipcc unrolls the loop of a callee before it inlines it and then computes all NIT rows ahead of the
// caller's branch (gemm256x192_kernel<float>: 56 spilled registers); pasted in, the loop unrolls with the kernel's own.
#define RES_PREFETCH(TO, NT, NCH, NIT, rv, res, res_ld, res_mod, res_rep, res_map, M, tid, m0, n0) \
  _Pragma("unroll") for (int it_ = 0; it_ < (NIT); ++it_) { \
    const int idx_ = (tid) + it_ * (NT); \
    const int row_ = idx_ / (NCH), ch_ = idx_ - row_ * (NCH); \
    int m_ = (m0) + row_; \
    m_ = m_ < (M) ? m_ : (M) - 1; \
    const size_t rpix_ = res_row(m_, res_mod, res_rep, res_map); \
    rv[it_] = *reinterpret_cast<const u32x4*>((res) + (rpix_ * (res_ld) + (n0) + ch_ * (16 / (int)sizeof(TO))) * (int)sizeof(TO)); \
  }

// Finish a chunk read from the LDS tile: y = TO(act2(float(t) + res)).  Returns false, with cv as read and a untouched, when
// there is neither a residual nor act_after_res (no unpack / pack round trip); otherwise a holds the finished values as floats.
template <typename TO, bool FAST, typename Res>
__device__ __forceinline__ bool finish_chunk(u32x4& cv, float (&a)[16 / sizeof(TO)], const Res& res, int act_after_res, int act) {
  constexpr int OVEC = 16 / sizeof(TO);
  if (!(res.has() || act_after_res)) return false;
  unpack16<TO>(cv, a);
  if (res.has()) {
    float r[OVEC];
    unpack16<TO>(res.chunk(), r);
#pragma unroll
    for (int e = 0; e < OVEC; ++e) a[e] += r[e];
  }
  if (act_after_res) {
#pragma unroll
    for (int e = 0; e < OVEC; ++e) a[e] = act_apply<FAST>(a[e], act);
  }
  cv = pack16<TO>(a);
  return true;
}

// Store the chunk of columns n.. (of N) at yp: finished and stored whole, or (TAIL kernels, when the row ends inside the chunk) the
// ragged channel tail element by element.  Returns finish_chunk's answer (false for a tail).
template <typename TO, bool FAST, bool TAIL, typename Res>
__device__ __forceinline__ bool store_out_chunk(char* yp, u32x4 cv, float (&a)[16 / sizeof(TO)], int n, int N, const Res& res, int act_after_res, int act) {
  constexpr int OVEC = 16 / sizeof(TO);
  if (!TAIL || n + OVEC <= N) {
    const bool fin = finish_chunk<TO, FAST>(cv, a, res, act_after_res, act);
    *reinterpret_cast<u32x4*>(yp) = cv;
    return fin;
  }
  if constexpr (TAIL) {
    unpack16<TO>(cv, a);
#pragma unroll
    for (int e = 0; e < OVEC; ++e) {
      if (n + e < N) {
        float av = a[e];
        if (res.has()) av += (float)res.ptr()[e];
        if (act_after_res) av = act_apply<FAST>(av, act);
        reinterpret_cast<TO*>(yp)[e] = (TO)av;
      }
    }
  }
  return false;
}
