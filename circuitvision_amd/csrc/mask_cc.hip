// Hole and sprinkle removal on SAM 2 mask logits (SAM2Transforms.postprocess_masks with max_hole_area / max_sprinkle_area > 0,
// sam2_infer.py:88-128): 8-connected components of BOTH phases of N f32 planes [N, h, w] -- foreground x > t, background x <= t -- in four
// launches on one stream, with no device-wide barrier:
//   tile      one workgroup per 64 x 64 tile: x is read once, the phase goes to LDS, the min-root union-find (common.hpp) runs in LDS over the
//             W, N, NW, NE neighbours of the same phase, and every pixel's tile-local root is written as a packed global index
//             (n * h * w + y * w + x).  Per pixel one coalesced read and two coalesced writes (root, area slot = 0); no global atomic.
//   seam      the pixels on a tile's first row link to the three pixels above them, those on a tile's first column to the three pixels to
//             their left (the diagonals and the one diagonal across a four-tile corner included), in global memory.
//   flatten   one workgroup per tile: pixels are counted per tile-local root in LDS (one LDS add per run of a row), each (tile, root)
//             finds its final root once and adds its count to that root's area slot, and every pixel's slot gets the final root.
//   apply     y = t + 10 / t - 10 / x from the root's area, or the labels (1 + the raster-first pixel of the component) and the areas.
// A root is the smallest packed index of its set, so labels do not depend on the order in which the unions happen.
// The tile and seam kernels are templates on the pixel source: x > t on f32 logits (above), or byte != 0 on u8 planes for cvmi_mask_remove_small --
// upstream's remove_small_regions (sam2/utils/amg.py) in place: label, fill the small background components (holes), label AGAIN (a filled hole
// can join foreground components), remove the small foreground components (islands) but the largest where every one is small.
#include <algorithm>

#include "common.hpp"

namespace {

constexpr int T = CVMI_MASK_CC_TILE, TT = T * T, NT = 256, PER = TT / NT;
static_assert(T == 64, "a wave is one tile row: the run counting in mask_cc_flatten_kernel relies on it");
constexpr int PH_NONE = 2;                    // a tile pixel outside the plane: no phase, never linked

struct TileAt {
  int base, x0, y0;                           // n * h * w; the tile's first pixel
};
__device__ __forceinline__ TileAt tile_at(int tile, int h, int w, int tiles_x, int tiles_y) {
  const int per = tiles_x * tiles_y, n = tile / per, r = tile - n * per, ty = r / tiles_x;
  return TileAt{n * h * w, (r - ty * tiles_x) * T, ty * T};
}

// the pixel source of the labelling: foreground is x > t on f32 logits, or a non-zero byte on u8 planes
struct LogitSrc {
  const float* x;
  float thresh;
  __device__ __forceinline__ bool operator()(int p) const { return x[p] > thresh; }
};
struct ByteSrc {
  const uint8_t* m;
  __device__ __forceinline__ bool operator()(int p) const { return m[p] != 0; }
};

template <typename Src>
__global__ __launch_bounds__(NT) void mask_cc_tile_kernel(Src fg, int* __restrict__ parent, int* __restrict__ area, int h, int w, int tiles_x, int tiles_y) {
  __shared__ int lab[TT];
  __shared__ uint8_t ph[TT];
  const TileAt t = tile_at(blockIdx.x, h, w, tiles_x, tiles_y);
  for (int i = threadIdx.x; i < TT; i += NT) {
    const int gx = t.x0 + (i & (T - 1)), gy = t.y0 + i / T;
    ph[i] = gx < w && gy < h ? (uint8_t)fg(t.base + gy * w + gx) : (uint8_t)PH_NONE;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TT; i += NT) {                       // the W link costs no union: a pixel starts as the child of its left neighbour
    const int f = ph[i];
    lab[i] = (i & (T - 1)) && f != PH_NONE && ph[i - 1] == f ? i - 1 : i;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TT; i += NT) {
    const int f = ph[i], lx = i & (T - 1), up = i - T;
    if (f == PH_NONE || up < 0) continue;
    if (ph[up] == f) {                                               // N: NW and NE of this phase already hang on N through their row
      uf_union(lab, i, up);
    } else {
      if (lx > 0 && ph[up - 1] == f && ph[i - 1] != f) uf_union(lab, i, up - 1);      // (W of this phase: W links to NW, its own N)
      if (lx + 1 < T && ph[up + 1] == f) uf_union(lab, i, up + 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TT; i += NT) {
    if (ph[i] == PH_NONE) continue;
    const int r = uf_find(lab, i);
    const int p = t.base + (t.y0 + i / T) * w + t.x0 + (i & (T - 1));
    parent[p] = t.base + (t.y0 + r / T) * w + t.x0 + (r & (T - 1));
    area[p] = 0;
  }
}

template <typename Src>
__global__ __launch_bounds__(NT) void mask_cc_seam_kernel(Src fg, int* __restrict__ parent, int N, int h, int w, int row_seams, int col_seams) {
  const int on_rows = row_seams * w, per = on_rows + col_seams * h;
  const long long total = (long long)N * per;
  for (long long idx = (long long)blockIdx.x * NT + threadIdx.x; idx < total; idx += (long long)gridDim.x * NT) {
    const int n = (int)(idx / per), base = n * h * w;
    int s = (int)(idx - (long long)n * per);
    if (s < on_rows) {                                               // first row of a tile: the three pixels above
      const int k = s / w, px = s - k * w, p = base + (k + 1) * T * w + px;
      const bool f = fg(p);
      for (int d = -1; d <= 1; ++d)
        if (px + d >= 0 && px + d < w && fg(p - w + d) == f) uf_union(parent, p, p - w + d);
    } else {                                                         // first column of a tile: the three pixels to the left
      s -= on_rows;
      const int k = s / h, py = s - k * h, p = base + py * w + (k + 1) * T;
      const bool f = fg(p);
      for (int d = -1; d <= 1; ++d)
        if (py + d >= 0 && py + d < h && fg(p - 1 + d * w) == f) uf_union(parent, p, p - 1 + d * w);
    }
  }
}

__global__ __launch_bounds__(NT) void mask_cc_flatten_kernel(int* __restrict__ parent, int* __restrict__ area, int h, int w, int tiles_x, int tiles_y) {
  __shared__ int cnt[TT];                                            // per tile-local root: its pixel count, then its final root
  const TileAt t = tile_at(blockIdx.x, h, w, tiles_x, tiles_y);
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < TT; i += NT) cnt[i] = 0;
  __syncthreads();
  int slot[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {                                    // (every lane takes every round: the shuffle and the ballot see whole rows)
    const int i = k * NT + threadIdx.x, gx = t.x0 + (i & (T - 1)), gy = t.y0 + i / T;
    int s = -1;
    if (gx < w && gy < h) {
      // the slot the tile pass wrote: this tile's root of the pixel; a root that a seam has since hung on a pixel outside the tile counts
      // under itself, one hung on a pixel of this tile under that one -- which has the same final root
      const int q = ld_relaxed(parent + t.base + gy * w + gx) - t.base, qy = q / w - t.y0, qx = q - (q / w) * w - t.x0;
      s = qx >= 0 && qx < T && qy >= 0 && qy < T ? qy * T + qx : i;
    }
    slot[k] = s;
    const int left = __shfl_up(s, 1);                                // (unconditionally: a lane that skipped the shuffle would hand its neighbour nothing)
    const bool head = lane == 0 || left != s;                        // one LDS add per run of equal slots in the row
    const unsigned long long above = (__ballot(head) >> lane) >> 1;
    if (head && s >= 0) atomicAdd(&cnt[s], above ? __ffsll(above) : 64 - lane);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TT; i += NT) {
    const int c = cnt[i];
    if (c > 0) {
      const int r = uf_find(parent, t.base + (t.y0 + i / T) * w + t.x0 + (i & (T - 1)));
      atomicAdd(area + r, c);
      cnt[i] = r;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = k * NT + threadIdx.x;
    if (slot[k] >= 0)                                                // (another tile's walk may pass through this slot: the final root is one of its ancestors)
      __hip_atomic_store(parent + t.base + (t.y0 + i / T) * w + t.x0 + (i & (T - 1)), cnt[slot[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <bool FILL>
__global__ __launch_bounds__(NT) void mask_cc_apply_kernel(const float* __restrict__ x, const int* __restrict__ parent, const int* __restrict__ area,
                                                           int total, int hw, float thresh, float max_hole, float max_sprinkle, float* __restrict__ y,
                                                           int* __restrict__ labels, int* __restrict__ areas) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int r = parent[i], a = area[r];
    if (FILL) {
      const float v = x[i];
      float o = v;
      if (v > thresh) {
        if (max_sprinkle > 0.f && (float)a <= max_sprinkle) o = thresh - 10.f;
      } else if (max_hole > 0.f && (float)a <= max_hole) {
        o = thresh + 10.f;
      }
      y[i] = o;
    } else {
      labels[i] = r % hw + 1;
      areas[i] = a;
    }
  }
}

int grid_for(long long n) { return (int)std::min<long long>(cdiv(n, NT), 1 << 16); }

struct Shape {
  int total, tiles_x, tiles_y;
};
// 0 when the planes cannot be labelled with int32 indices
bool shape_of(int N, int h, int w, Shape& s) {
  if (N <= 0 || h <= 0 || w <= 0 || (long long)N * h * w >= (1ll << 31)) return false;
  s = Shape{N * h * w, cdiv(w, T), cdiv(h, T)};
  return true;
}

// tile + seam + flatten: afterwards parent[p] is the root of p and area[root] the size of its component
template <typename Src> int label_planes(Src fg, int N, int h, int w, const Shape& sh, int* parent, int* area, hipStream_t s) {
  const int tiles = N * sh.tiles_x * sh.tiles_y;                     // <= N * h * w
  hipLaunchKernelGGL(mask_cc_tile_kernel<Src>, dim3(tiles), dim3(NT), 0, s, fg, parent, area, h, w, sh.tiles_x, sh.tiles_y);
  const long long seam = (long long)N * ((long long)(sh.tiles_y - 1) * w + (long long)(sh.tiles_x - 1) * h);
  if (seam > 0)
    hipLaunchKernelGGL(mask_cc_seam_kernel<Src>, dim3(grid_for(seam)), dim3(NT), 0, s, fg, parent, N, h, w, sh.tiles_y - 1, sh.tiles_x - 1);
  hipLaunchKernelGGL(mask_cc_flatten_kernel, dim3(tiles), dim3(NT), 0, s, parent, area, h, w, sh.tiles_x, sh.tiles_y);
  CVMI_LAUNCH_CHECK();
  return 0;
}

// ---- cvmi_mask_remove_small: the two apply passes on u8 planes ---------------------------------------------------------------------------------
constexpr int RS_PER = 16, RS_CHUNK = NT * RS_PER;                   // pixels of one plane per workgroup
enum { INFO_CHANGED, INFO_AREA, INFO_X0, INFO_Y0, INFO_X1, INFO_Y1, INFO_FILLED, INFO_REMOVED, INFO_N };

__global__ __launch_bounds__(NT) void remove_init_kernel(int* __restrict__ info, unsigned long long* __restrict__ best, int N, int h, int w) {
  const int n = blockIdx.x * NT + threadIdx.x;
  if (n >= N) return;
  const int init[INFO_N] = {0, 0, w, h, -1, -1, 0, 0};
  for (int k = 0; k < INFO_N; ++k) info[n * INFO_N + k] = init[k];
  best[n] = 0ull;
}

// per plane: the maximum over the foreground roots of (area << 32 | ~(root's index within the plane)) -- the largest component, the raster-first
// one among equals.  An integer maximum: the result does not depend on the order of the atomics.
__global__ __launch_bounds__(NT) void remove_best_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ parent, const int* __restrict__ area,
                                                         int total, int hw, unsigned long long* __restrict__ best) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    if (parent[i] != (int)i || mask[i] == 0) continue;
    const int n = (int)(i / hw);
    atomicMax(best + n, ((unsigned long long)(unsigned)area[i] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)((int)i - n * hw)));
  }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v = min(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v = max(v, __shfl_xor(v, d));
  return v;
}

// ISLANDS = false: a background pixel of a component below min_area becomes 255.  true: a foreground pixel of a component below min_area becomes 0,
// unless every foreground component of the plane is that small and this one is the plane's `best`.  `last`: also the final plane's area and extent.
template <bool ISLANDS>
__global__ __launch_bounds__(NT) void remove_apply_kernel(uint8_t* __restrict__ mask, const int* __restrict__ parent, const int* __restrict__ area, int hw,
                                                          int w, int chunks, int min_area, const unsigned long long* __restrict__ best,
                                                          int* __restrict__ info, int last) {
  const int n = blockIdx.x / chunks, c = blockIdx.x - n * chunks, base = n * hw;
  int keep_root = -1;
  if (ISLANDS) {
    const unsigned long long b = best[n];
    if (b != 0ull && (int)(b >> 32) < min_area) keep_root = base + (int)(0xFFFFFFFFu - (unsigned)b);      // (0: a plane without foreground)
  }
  int changed = 0, cnt = 0, x0 = w, y0 = hw, x1 = -1, y1 = -1;
#pragma unroll 4
  for (int k = 0; k < RS_PER; ++k) {
    const int i = c * RS_CHUNK + k * NT + threadIdx.x;
    if (i >= hw) break;
    uint8_t v = mask[base + i];
    const bool on = v != 0;
    if (on == ISLANDS) {
      const int r = parent[base + i];
      if (area[r] < min_area && r != keep_root) {
        v = ISLANDS ? 0 : 255;
        mask[base + i] = v;
        ++changed;
      }
    }
    if (last && v != 0) {
      const int y = i / w, x = i - y * w;
      ++cnt;
      x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x); y1 = max(y1, y);
    }
  }
  changed = wave_sum(changed);
  if (last) {
    cnt = wave_sum(cnt); x0 = wave_min(x0); y0 = wave_min(y0); x1 = wave_max(x1); y1 = wave_max(y1);
  }
  if ((threadIdx.x & 63) == 0) {
    int* o = info + n * INFO_N;
    if (changed) atomicAdd(o + (ISLANDS ? INFO_REMOVED : INFO_FILLED), changed);
    if (last && cnt) {
      atomicAdd(o + INFO_AREA, cnt);
      atomicMin(o + INFO_X0, x0); atomicMin(o + INFO_Y0, y0); atomicMax(o + INFO_X1, x1); atomicMax(o + INFO_Y1, y1);
    }
  }
}

__global__ __launch_bounds__(NT) void remove_finish_kernel(int* __restrict__ info, int N) {
  const int n = blockIdx.x * NT + threadIdx.x;
  if (n >= N) return;
  int* o = info + n * INFO_N;
  o[INFO_CHANGED] = (o[INFO_FILLED] | o[INFO_REMOVED]) != 0;
  if (o[INFO_AREA] == 0) o[INFO_X0] = o[INFO_Y0] = o[INFO_X1] = o[INFO_Y1] = 0;      // upstream's batched_mask_to_box on an empty mask
}

}  // namespace

extern "C" size_t cvmi_mask_cc_workspace(int N, int h, int w) {
  Shape sh;
  return shape_of(N, h, w, sh) ? 2 * sizeof(int) * (size_t)sh.total : 0;
}

extern "C" int cvmi_mask_components(const float* x, int N, int h, int w, float thresh, int* labels, int* areas, void* workspace, cvmi_stream_t stream_) {
  Shape sh;
  CVMI_CHECK(shape_of(N, h, w, sh), "mask_components: %d planes of %d x %d: sizes must be positive and N * h * w below 2^31", N, h, w);
  CVMI_CHECK(x && labels && areas && workspace && ((uintptr_t)workspace & 3) == 0, "mask_components: bad arguments");
  hipStream_t s = (hipStream_t)stream_;
  int *parent = (int*)workspace, *area = parent + sh.total;
  if (label_planes(LogitSrc{x, thresh}, N, h, w, sh, parent, area, s)) return 1;
  hipLaunchKernelGGL(mask_cc_apply_kernel<false>, dim3(grid_for(sh.total)), dim3(NT), 0, s, x, parent, area, sh.total, h * w, thresh, 0.f, 0.f, nullptr,
                     labels, areas);
  CVMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int cvmi_mask_fill_small(const float* x, int N, int h, int w, float thresh, float max_hole_area, float max_sprinkle_area, float* y,
                                    void* workspace, cvmi_stream_t stream_) {
  Shape sh;
  CVMI_CHECK(shape_of(N, h, w, sh), "mask_fill_small: %d planes of %d x %d: sizes must be positive and N * h * w below 2^31", N, h, w);
  CVMI_CHECK(x && y && workspace && ((uintptr_t)workspace & 3) == 0, "mask_fill_small: bad arguments");
  const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y, bytes = sizeof(float) * (uintptr_t)sh.total;
  CVMI_CHECK(ya + bytes <= xa || xa + bytes <= ya, "mask_fill_small: y must not alias x");
  hipStream_t s = (hipStream_t)stream_;
  int *parent = (int*)workspace, *area = parent + sh.total;
  if (label_planes(LogitSrc{x, thresh}, N, h, w, sh, parent, area, s)) return 1;
  hipLaunchKernelGGL(mask_cc_apply_kernel<true>, dim3(grid_for(sh.total)), dim3(NT), 0, s, x, parent, area, sh.total, h * w, thresh, max_hole_area,
                     max_sprinkle_area, y, nullptr, nullptr);
  CVMI_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t cvmi_mask_remove_small_workspace(int N, int H, int W) {
  Shape sh;
  return shape_of(N, H, W, sh) ? sizeof(unsigned long long) * (size_t)N + 2 * sizeof(int) * (size_t)sh.total : 0;
}

extern "C" int cvmi_mask_remove_small(uint8_t* mask, int N, int H, int W, int min_area, int phases, int* info, void* workspace, cvmi_stream_t stream_) {
  Shape sh;
  CVMI_CHECK(shape_of(N, H, W, sh), "mask_remove_small: %d planes of %d x %d: sizes must be positive and N * H * W below 2^31", N, H, W);
  CVMI_CHECK(min_area > 0 && phases >= 1 && phases <= 3, "mask_remove_small: min_area = %d must be positive and phases = %d one of 1 (holes), 2 (islands), 3 (both)",
             min_area, phases);
  CVMI_CHECK(mask && info && workspace && ((uintptr_t)workspace & 7) == 0, "mask_remove_small: bad arguments (null pointer, or workspace not 8-byte aligned)");
  hipStream_t s = (hipStream_t)stream_;
  unsigned long long* best = (unsigned long long*)workspace;
  int *parent = (int*)(best + N), *area = parent + sh.total;
  const int hw = H * W, chunks = cdiv(hw, RS_CHUNK);                   // N * chunks <= N * H * W
  hipLaunchKernelGGL(remove_init_kernel, dim3(cdiv(N, NT)), dim3(NT), 0, s, info, best, N, H, W);
  if (phases & 1) {
    if (label_planes(ByteSrc{mask}, N, H, W, sh, parent, area, s)) return 1;
    hipLaunchKernelGGL(remove_apply_kernel<false>, dim3(N * chunks), dim3(NT), 0, s, mask, parent, area, hw, W, chunks, min_area, best, info, phases == 1);
  }
  if (phases & 2) {
    if (label_planes(ByteSrc{mask}, N, H, W, sh, parent, area, s)) return 1;
    hipLaunchKernelGGL(remove_best_kernel, dim3(grid_for(sh.total)), dim3(NT), 0, s, mask, parent, area, sh.total, hw, best);
    hipLaunchKernelGGL(remove_apply_kernel<true>, dim3(N * chunks), dim3(NT), 0, s, mask, parent, area, hw, W, chunks, min_area, best, info, 1);
  }
  hipLaunchKernelGGL(remove_finish_kernel, dim3(cdiv(N, NT)), dim3(NT), 0, s, info, N);
  CVMI_LAUNCH_CHECK();
  return 0;
}
