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

__global__ __launch_bounds__(NT) void mask_cc_tile_kernel(const float* __restrict__ x, int* __restrict__ parent, int* __restrict__ area, int h, int w,
                                                          int tiles_x, int tiles_y, float thresh) {
  __shared__ int lab[TT];
  __shared__ uint8_t ph[TT];
  const TileAt t = tile_at(blockIdx.x, h, w, tiles_x, tiles_y);
  for (int i = threadIdx.x; i < TT; i += NT) {
    const int gx = t.x0 + (i & (T - 1)), gy = t.y0 + i / T;
    ph[i] = gx < w && gy < h ? (uint8_t)(x[t.base + gy * w + gx] > thresh) : (uint8_t)PH_NONE;
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

__global__ __launch_bounds__(NT) void mask_cc_seam_kernel(const float* __restrict__ x, int* __restrict__ parent, int N, int h, int w, int row_seams,
                                                          int col_seams, float thresh) {
  const int on_rows = row_seams * w, per = on_rows + col_seams * h;
  const long long total = (long long)N * per;
  for (long long idx = (long long)blockIdx.x * NT + threadIdx.x; idx < total; idx += (long long)gridDim.x * NT) {
    const int n = (int)(idx / per), base = n * h * w;
    int s = (int)(idx - (long long)n * per);
    if (s < on_rows) {                                               // first row of a tile: the three pixels above
      const int k = s / w, px = s - k * w, p = base + (k + 1) * T * w + px;
      const bool f = x[p] > thresh;
      for (int d = -1; d <= 1; ++d)
        if (px + d >= 0 && px + d < w && (x[p - w + d] > thresh) == f) uf_union(parent, p, p - w + d);
    } else {                                                         // first column of a tile: the three pixels to the left
      s -= on_rows;
      const int k = s / h, py = s - k * h, p = base + py * w + (k + 1) * T;
      const bool f = x[p] > thresh;
      for (int d = -1; d <= 1; ++d)
        if (py + d >= 0 && py + d < h && (x[p - 1 + d * w] > thresh) == f) uf_union(parent, p, p - 1 + d * w);
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
int label_planes(const float* x, int N, int h, int w, float thresh, const Shape& sh, int* parent, int* area, hipStream_t s) {
  const int tiles = N * sh.tiles_x * sh.tiles_y;                     // <= N * h * w
  hipLaunchKernelGGL(mask_cc_tile_kernel, dim3(tiles), dim3(NT), 0, s, x, parent, area, h, w, sh.tiles_x, sh.tiles_y, thresh);
  const long long seam = (long long)N * ((long long)(sh.tiles_y - 1) * w + (long long)(sh.tiles_x - 1) * h);
  if (seam > 0)
    hipLaunchKernelGGL(mask_cc_seam_kernel, dim3(grid_for(seam)), dim3(NT), 0, s, x, parent, N, h, w, sh.tiles_y - 1, sh.tiles_x - 1, thresh);
  hipLaunchKernelGGL(mask_cc_flatten_kernel, dim3(tiles), dim3(NT), 0, s, parent, area, h, w, sh.tiles_x, sh.tiles_y);
  CVMI_LAUNCH_CHECK();
  return 0;
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
  if (label_planes(x, N, h, w, thresh, sh, parent, area, s)) return 1;
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
  if (label_planes(x, N, h, w, thresh, sh, parent, area, s)) return 1;
  hipLaunchKernelGGL(mask_cc_apply_kernel<true>, dim3(grid_for(sh.total)), dim3(NT), 0, s, x, parent, area, sh.total, h * w, thresh, max_hole_area,
                     max_sprinkle_area, y, nullptr, nullptr);
  CVMI_LAUNCH_CHECK();
  return 0;
}
