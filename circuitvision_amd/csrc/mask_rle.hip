// Uncompressed run-length encoding of N binary u8 planes [N, H, W] (upstream sam2/utils/amg.py mask_to_rle_pytorch): the plane is read in
// COLUMN-major order (y fastest), the runs alternate and start with a run of zeros (0 when pixel (0, 0) is set), a run goes on across a
// column end, and the runs of a plane sum to H * W.  Four launches on one stream, every position from a prefix sum:
//   bits      one workgroup per 64 x 64 tile: the bytes are read once (4 per lane where W % 4 == 0), staged in LDS, and every tile column is
//             balloted into one 64-bit word of the transposed bit-plane  bits[n][x][b]  (b = y / 64; bit y % 64; 0 past the plane's last row).
//             In that layout the column-major scan order of a plane is the order of its words.
//   reduce    one lane per word: its transitions  t = (w ^ (w << 1 | carry)) & valid  (carry = the pixel before the word in scan order, 0 at
//             a plane's start), their count (+ 1 for a plane's last word: the closing run) and the packed position of its last transition,
//             reduced per 256 words to one (sum, max) pair.
//   scan      one workgroup: exclusive scan of the pairs; the total is offsets[N].
//   emit      one lane per word again: the same pair scanned within the workgroup gives the word's first output slot and the transition
//             before it; every transition writes  position - previous position, a plane's last word also H * W - the last position, and a
//             plane's first word offsets[n].  Nothing is written at or past counts[cap_runs].
#include "common.hpp"

namespace {

constexpr int T = 64, NT = 256, LDW = T / 4 + 1;   // a tile row in LDS: 16 words of 4 pixels + 1 (the column reads of a wave spread over the banks)

struct Pair {
  int cnt, last;                                   // transitions (and closing runs); 1 + the packed position of the last transition, 0 = none
};
__device__ __forceinline__ Pair join(Pair a, Pair b) { return Pair{a.cnt + b.cnt, a.last > b.last ? a.last : b.last}; }

struct Geo {
  int H, W, HB, per_plane;                         // HB = words per column, per_plane = W * HB
  long long units;                                 // N * per_plane
};

template <bool VEC4>
__global__ __launch_bounds__(NT) void rle_bits_kernel(const uint8_t* __restrict__ mask, unsigned long long* __restrict__ bits, int H, int W, int tiles_x,
                                                      int tiles_y) {
  __shared__ uint32_t tile[T * LDW];
  const int per = tiles_x * tiles_y, n = blockIdx.x / per, r = blockIdx.x - n * per, ty = r / tiles_x, x0 = (r - ty * tiles_x) * T, y0 = ty * T;
  const uint8_t* plane = mask + (size_t)n * H * W;
  if (VEC4) {                                      // 16 lanes per row, 4 bytes each; W % 4 == 0 keeps a word inside its row
    for (int i = threadIdx.x; i < T * (T / 4); i += NT) {
      const int row = i / (T / 4), c4 = i - row * (T / 4), gy = y0 + row, gx = x0 + 4 * c4;
      tile[row * LDW + c4] = gy < H && gx < W ? *(const uint32_t*)(plane + (size_t)gy * W + gx) : 0u;
    }
  } else {
    uint8_t* tb = (uint8_t*)tile;
    for (int i = threadIdx.x; i < T * T; i += NT) {
      const int row = i / T, c = i - row * T, gy = y0 + row, gx = x0 + c;
      tb[row * (4 * LDW) + c] = gy < H && gx < W ? plane[(size_t)gy * W + gx] : (uint8_t)0;
    }
  }
  __syncthreads();
  const uint8_t* tb = (const uint8_t*)tile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, HB = tiles_y;
  unsigned long long mine = 0;
#pragma unroll
  for (int j = 0; j < T / 4; ++j) {                // a wave takes 16 columns; lane = the row
    const unsigned long long word = __ballot(tb[lane * (4 * LDW) + wave * (T / 4) + j] != 0);
    if (lane == j) mine = word;
  }
  const int gx = x0 + wave * (T / 4) + lane;
  if (lane < T / 4 && gx < W) bits[((size_t)n * W + gx) * HB + ty] = mine;
}

// the word's transitions and its scan element
__device__ __forceinline__ Pair unit_pair(const unsigned long long* __restrict__ bits, long long u, const Geo& g, unsigned long long& t, int& base) {
  const int n = (int)(u / g.per_plane), r = (int)(u - (long long)n * g.per_plane), x = r / g.HB, b = r - x * g.HB;
  const unsigned long long w = bits[u];
  unsigned long long carry = 0;
  if (r > 0) carry = (bits[u - 1] >> (b > 0 ? 63 : (g.H - 1) & 63)) & 1ull;       // the word before: this column's, or the previous column's last
  const int valid = g.H - b * 64 < 64 ? g.H - b * 64 : 64;
  t = (w ^ ((w << 1) | carry)) & (valid == 64 ? ~0ull : (1ull << valid) - 1ull);
  base = n * g.H * g.W + x * g.H + b * 64;         // packed position of the word's bit 0
  return Pair{(int)__popcll(t) + (r == g.per_plane - 1 ? 1 : 0), t ? base + 64 - (int)__clzll((long long)t) : 0};
}

// exclusive scan of one Pair per thread over the workgroup; `total` = the workgroup's sum, in every thread
__device__ __forceinline__ Pair block_scan(Pair v, Pair& total) {
  __shared__ Pair part[NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Pair inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const Pair o{__shfl_up(inc.cnt, d), __shfl_up(inc.last, d)};
    if (lane >= d) inc = join(o, inc);
  }
  __syncthreads();                                 // (part is reused by the next call)
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  Pair before{0, 0};
  total = Pair{0, 0};
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) {
    if (k < wave) before = join(before, part[k]);
    total = join(total, part[k]);
  }
  Pair exc{__shfl_up(inc.cnt, 1), __shfl_up(inc.last, 1)};
  if (lane == 0) exc = Pair{0, 0};
  return join(before, exc);
}

__global__ __launch_bounds__(NT) void rle_reduce_kernel(const unsigned long long* __restrict__ bits, Geo g, Pair* __restrict__ agg) {
  const long long u = (long long)blockIdx.x * NT + threadIdx.x;
  Pair v{0, 0};
  if (u < g.units) {
    unsigned long long t;
    int base;
    v = unit_pair(bits, u, g, t, base);
  }
  Pair total;
  block_scan(v, total);
  if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

__global__ __launch_bounds__(NT) void rle_scan_kernel(Pair* __restrict__ agg, int blocks, int* __restrict__ offsets, int N) {
  Pair carry{0, 0};
  for (int base = 0; base < blocks; base += NT) {
    const int i = base + threadIdx.x;
    Pair total;
    const Pair exc = block_scan(i < blocks ? agg[i] : Pair{0, 0}, total);
    if (i < blocks) agg[i] = join(carry, exc);
    carry = join(carry, total);
  }
  if (threadIdx.x == 0) offsets[N] = carry.cnt;
}

__global__ __launch_bounds__(NT) void rle_emit_kernel(const unsigned long long* __restrict__ bits, Geo g, const Pair* __restrict__ agg, int cap,
                                                      int* __restrict__ offsets, int* __restrict__ counts) {
  const long long u = (long long)blockIdx.x * NT + threadIdx.x;
  Pair v{0, 0};
  unsigned long long t = 0;
  int base = 0;
  if (u < g.units) v = unit_pair(bits, u, g, t, base);
  Pair total;
  const Pair exc = join(agg[blockIdx.x], block_scan(v, total));
  if (u >= g.units) return;
  const int n = (int)(u / g.per_plane), r = (int)(u - (long long)n * g.per_plane), hw = g.H * g.W, plane0 = n * hw;
  int slot = exc.cnt, prev = exc.last > plane0 ? exc.last - 1 : plane0;              // packed; a transition of an earlier plane does not count
  if (r == 0) offsets[n] = slot;
  while (t) {
    const int pos = base + __ffsll((long long)t) - 1;
    t &= t - 1;
    if (slot < cap) counts[slot] = pos - prev;
    prev = pos;
    ++slot;
  }
  if (r == g.per_plane - 1 && slot < cap) counts[slot] = plane0 + hw - prev;
}

// false when the planes cannot be encoded with int32 positions and totals (a plane has at most H * W + 1 runs)
bool geo_of(int N, int H, int W, Geo& g) {
  if (N <= 0 || H <= 0 || W <= 0 || (long long)N * H * W + N >= (1ll << 31)) return false;
  g.H = H;
  g.W = W;
  g.HB = cdiv(H, T);
  g.per_plane = W * g.HB;
  g.units = (long long)N * g.per_plane;
  return true;
}
size_t bits_bytes(const Geo& g) { return sizeof(unsigned long long) * (size_t)g.units; }

}  // namespace

extern "C" size_t cvmi_mask_rle_workspace(int N, int H, int W) {
  Geo g;
  return geo_of(N, H, W, g) ? bits_bytes(g) + sizeof(Pair) * (size_t)cdiv(g.units, NT) : 0;
}

extern "C" int cvmi_mask_rle(const uint8_t* mask, int N, int H, int W, int cap_runs, int* offsets, int* counts, void* workspace, size_t workspace_bytes,
                             cvmi_stream_t stream_) {
  Geo g;
  CVMI_CHECK(geo_of(N, H, W, g), "mask_rle: %d planes of %d x %d: sizes must be positive and N * H * W + N below 2^31", N, H, W);
  CVMI_CHECK(mask && offsets && workspace && ((uintptr_t)workspace & 7) == 0 && cap_runs >= 0 && (counts || cap_runs == 0),
             "mask_rle: bad arguments (null pointer, workspace not 8-byte aligned, or counts = NULL with cap_runs = %d)", cap_runs);
  const size_t need = cvmi_mask_rle_workspace(N, H, W);
  CVMI_CHECK(workspace_bytes >= need, "mask_rle: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream_;
  unsigned long long* bits = (unsigned long long*)workspace;
  Pair* agg = (Pair*)((char*)workspace + bits_bytes(g));
  const int tiles_x = cdiv(W, T), tiles_y = g.HB, tiles = N * tiles_x * tiles_y, blocks = cdiv(g.units, NT);
  if (W % 4 == 0 && ((uintptr_t)mask & 3) == 0)
    hipLaunchKernelGGL(rle_bits_kernel<true>, dim3(tiles), dim3(NT), 0, s, mask, bits, H, W, tiles_x, tiles_y);
  else
    hipLaunchKernelGGL(rle_bits_kernel<false>, dim3(tiles), dim3(NT), 0, s, mask, bits, H, W, tiles_x, tiles_y);
  hipLaunchKernelGGL(rle_reduce_kernel, dim3(blocks), dim3(NT), 0, s, bits, g, agg);
  hipLaunchKernelGGL(rle_scan_kernel, dim3(1), dim3(NT), 0, s, agg, blocks, offsets, N);
  hipLaunchKernelGGL(rle_emit_kernel, dim3(blocks), dim3(NT), 0, s, bits, g, agg, cap_runs, offsets, counts);
  CVMI_LAUNCH_CHECK();
  return 0;
}
