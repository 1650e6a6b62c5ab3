// Automatic mask generation (upstream SAM2AutomaticMaskGenerator at its defaults), the part behind the decoder: every candidate plane of a
// point-grid chunk scored at the image's own resolution WITHOUT the f32 map (cvmi_amg_score: three pixel counts and the bounding box of
// bilinear(low) against three levels, optionally the u8 mask), and one image's filter + ordered append of the kept candidates into its pool,
// its record list and the block cvmi_yolo_nms reads (cvmi_amg_select).  With crop layers (crop_n_layers > 0) a plane belongs to a crop of
// the image: the append also drops the candidates a crop border cuts (cvmi_amg_select_crop), and the survivors' masks are written into a
// window of a full-image plane (cvmi_amg_score_window).  f32 only: built once, no 16-bit operand type.
#include <algorithm>

#include "common.hpp"
#include "bilinear.hpp"

namespace {

// ---- cvmi_amg_score ------------------------------------------------------------------------------------------------------------------
// A workgroup owns units of ONE plane (blockIdx.y): a band of output rows x a chunk of output columns.  Per unit it stages the source
// rows x columns the unit's taps touch in LDS (a 4x up-scale: 10 rows for 32; the launch asks for the shape's bound, 12 KB there), builds the y table {tap row offsets, weight} once in LDS and
// each thread its 4 adjacent columns' x table in registers, then walks the band: 4 LDS reads + bil_mix per sample, the three counts and
// the mask's row / column occupancy in registers.  One wave reduction (__shfl_xor), one LDS round per workgroup, one integer atomic per
// value per workgroup.  Integer sums and extrema: the result does not depend on the launch.
constexpr int AMG_THREADS = 256;
constexpr int AMG_COLS = 4;                        // adjacent output columns per thread (one 4-byte mask store where W % 4 == 0)
constexpr int AMG_CHUNK = AMG_THREADS * AMG_COLS;  // widest column chunk of a unit
constexpr int AMG_BAND = 32;                       // output rows of a unit (more when a narrow plane leaves threads for more rows, fewer when LDS is short)
constexpr int AMG_GRID_CAP = 256;                  // workgroups per plane: the units past it are strided
constexpr int AMG_YTAB = 256;                      // longest band (= AMG_THREADS rows, at W <= 4)
constexpr int AMG_LDS_FLOATS = 12288;              // most a unit's staged source window may take: 48 KB (the launch asks for what the shape needs)

struct AmgShape {
  int txn_log2;   // threads across a row: 1 << txn_log2 (x 4 columns = the chunk), the other AMG_THREADS >> txn_log2 take rows
  int band;       // output rows per unit
  int nchunks, nbands;
  int lds_floats; // bound of a unit's staged window (rows x columns), the launch's dynamic LDS
};

// cvmi_amg_score_window: the mask planes are PH x PW and the resized H x W map sits at (x0, y0) in them.  The units then tile the PLANE (so a
// thread's 4 columns are an aligned word of it wherever the window starts); a unit stages and samples only its part of the window and
// writes zeros elsewhere.  cvmi_amg_score is the window that is the plane.
struct AmgWindow {
  int PH, PW, x0, y0;
};

__global__ void amg_init_kernel(int* __restrict__ stats, int M, int H, int W) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M) {
    int* s = stats + (size_t)i * 8;
    s[0] = 0; s[1] = 0; s[2] = 0; s[3] = W; s[4] = H; s[5] = -1; s[6] = -1; s[7] = 0;
  }
}

// upstream's batched_mask_to_box: the box of an empty mask is {0, 0, 0, 0}
__global__ void amg_finish_kernel(int* __restrict__ stats, int M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M && stats[(size_t)i * 8 + 5] < 0) {
    int* s = stats + (size_t)i * 8;
    s[3] = 0; s[4] = 0; s[5] = 0; s[6] = 0;
  }
}

// the mask bytes of a thread's 4 adjacent columns of one row: one 4-byte store where the plane's rows are word-aligned (VEC)
template <bool VEC>
__device__ __forceinline__ void amg_store4(uint8_t* __restrict__ mrow, unsigned row_on, const bool (&ok)[AMG_COLS]) {
  if (VEC) {                                                        // PW % 4 == 0 and the planes 4-byte aligned: the 4 columns are all inside, one store
    if (ok[0]) *reinterpret_cast<uint32_t*>(mrow) = ((row_on & 1u) ? 0xFFu : 0u) | ((row_on & 2u) ? 0xFF00u : 0u) | ((row_on & 4u) ? 0xFF0000u : 0u) | ((row_on & 8u) ? 0xFF000000u : 0u);
  } else {
#pragma unroll
    for (int k = 0; k < AMG_COLS; ++k)
      if (ok[k]) mrow[k] = ((row_on >> k) & 1u) ? 255 : 0;
  }
}

template <bool MASK, bool VEC, bool WIN>
__global__ __launch_bounds__(AMG_THREADS) void amg_score_kernel(const float* __restrict__ low, int h, int w, int H, int W, float sy, float sx,
                                                               float lo, float mid, float hi, AmgShape sh, AmgWindow win,
                                                               int* __restrict__ stats, uint8_t* __restrict__ mask) {
  extern __shared__ float tile[];
  __shared__ int yo0[AMG_YTAB], yo1[AMG_YTAB];
  __shared__ float yl[AMG_YTAB];
  __shared__ int red[AMG_THREADS / 64][7];
  const int tid = threadIdx.x, n = blockIdx.y;
  const int tx = tid & ((1 << sh.txn_log2) - 1), ty = tid >> sh.txn_log2, tyn = AMG_THREADS >> sh.txn_log2;
  const int chunk_w = AMG_COLS << sh.txn_log2;
  const float* pl = low + (size_t)n * h * w;
  // the plane the units tile and the map's origin in it; rows / columns of the MAP are plane rows / columns minus (wy0, wx0)
  const int PH = WIN ? win.PH : H, PW = WIN ? win.PW : W, wx0 = WIN ? win.x0 : 0, wy0 = WIN ? win.y0 : 0;
  uint8_t* mp = MASK ? mask + (size_t)n * PH * PW : nullptr;
  int n_hi = 0, n_lo = 0, area = 0, ex0 = W, ey0 = H, ex1 = -1, ey1 = -1;

  const int nunits = sh.nbands * sh.nchunks;
  for (int unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
    const int band = unit / sh.nchunks, chunk = unit - band * sh.nchunks;
    const int py0 = band * sh.band, nr = min(sh.band, PH - py0);
    const int c0 = chunk * chunk_w, nc = min(chunk_w, PW - c0);
    const int col0 = c0 + tx * AMG_COLS;
    bool ok[AMG_COLS];
#pragma unroll
    for (int k = 0; k < AMG_COLS; ++k) ok[k] = col0 + k < c0 + nc;
    // the unit's rows and columns of the map (all of them without a window)
    int ra = py0 - wy0, rb = ra + nr - 1, ca = c0 - wx0, cb = ca + nc - 1;
    if (WIN) {
      ra = max(ra, 0); rb = min(rb, H - 1); ca = max(ca, 0); cb = min(cb, W - 1);
      if (ra > rb || ca > cb) {                                       // a unit clear of the window: zeros, nothing staged (uniform over the workgroup)
        for (int r = ty; r < nr; r += tyn) amg_store4<VEC>(mp + (size_t)(py0 + r) * PW + col0, 0u, ok);
        continue;
      }
    }
    // the source window of the unit: taps are monotone in the destination index
    int ya, yb, xa, xb, t;
    float tl;
    bil_axis(ra, sy, h, ya, t, tl);
    bil_axis(rb, sy, h, t, yb, tl);
    bil_axis(ca, sx, w, xa, t, tl);
    bil_axis(cb, sx, w, t, xb, tl);
    const int ncols = xb - xa + 1, nrows = yb - ya + 1;
    __syncthreads();                                                  // the previous unit's reads of tile / the y table are over
    if (tid < nr) {
      int y0, y1;
      float ly;
      bil_axis(WIN ? min(max(py0 + tid - wy0, ra), rb) : py0 + tid, sy, h, y0, y1, ly);       // (a row off the window is not sampled)
      yo0[tid] = (y0 - ya) * ncols; yo1[tid] = (y1 - ya) * ncols; yl[tid] = ly;
    }
    for (int r = 0; r < nrows; ++r) {
      const float* src = pl + (size_t)(ya + r) * w + xa;
      for (int c = tid; c < ncols; c += AMG_THREADS) {
        const int at = r * ncols + c;
        if (at < sh.lds_floats) tile[at] = src[c];                   // (the host sized the LDS for the largest window: never false)
      }
    }
    int xo0[AMG_COLS], xo1[AMG_COLS];
    float lx[AMG_COLS];
    bool in[AMG_COLS];                                                // the column is counted: inside the chunk (and the window)
#pragma unroll
    for (int k = 0; k < AMG_COLS; ++k) {
      const int ox = col0 + k - wx0;
      in[k] = ok[k] && (!WIN || (ox >= 0 && ox < W));
      int x0, x1;
      bil_axis(WIN ? min(max(ox, 0), W - 1) : min(ox, W - 1), sx, w, x0, x1, lx[k]);
      xo0[k] = min(max(x0 - xa, 0), ncols - 1); xo1[k] = min(max(x1 - xa, 0), ncols - 1);       // (a column past the chunk reads inside the window; it is not counted)
    }
    __syncthreads();
    unsigned col_on = 0;
    for (int r = ty; r < nr; r += tyn) {
      const int oy = py0 + r - wy0;
      unsigned row_on = 0;
      if (!WIN || (oy >= 0 && oy < H)) {
        const int o0 = yo0[r], o1 = yo1[r];
        const float ly = yl[r];
#pragma unroll
        for (int k = 0; k < AMG_COLS; ++k) {
          const float v = bil_mix(tile[o0 + xo0[k]], tile[o0 + xo1[k]], tile[o1 + xo0[k]], tile[o1 + xo1[k]], ly, lx[k]);
          const bool on = in[k] && v > mid;
          n_hi += (in[k] && v > hi) ? 1 : 0;
          n_lo += (in[k] && v > lo) ? 1 : 0;
          area += on ? 1 : 0;
          row_on |= (on ? 1u : 0u) << k;
        }
      }
      col_on |= row_on;
      if (row_on) { ey0 = min(ey0, oy); ey1 = max(ey1, oy); }
      if (MASK) amg_store4<VEC>(mp + (size_t)(py0 + r) * PW + col0, row_on, ok);
    }
#pragma unroll
    for (int k = 0; k < AMG_COLS; ++k)
      if ((col_on >> k) & 1u) { ex0 = min(ex0, col0 + k - wx0); ex1 = max(ex1, col0 + k - wx0); }
  }

#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_hi += __shfl_xor(n_hi, off); n_lo += __shfl_xor(n_lo, off); area += __shfl_xor(area, off);
    ex0 = min(ex0, __shfl_xor(ex0, off)); ey0 = min(ey0, __shfl_xor(ey0, off));
    ex1 = max(ex1, __shfl_xor(ex1, off)); ey1 = max(ey1, __shfl_xor(ey1, off));
  }
  if ((tid & 63) == 0) {
    int* r = red[tid >> 6];
    r[0] = n_hi; r[1] = n_lo; r[2] = area; r[3] = ex0; r[4] = ey0; r[5] = ex1; r[6] = ey1;
  }
  __syncthreads();
  if (tid == 0) {
    for (int wv = 1; wv < AMG_THREADS / 64; ++wv) {
      n_hi += red[wv][0]; n_lo += red[wv][1]; area += red[wv][2];
      ex0 = min(ex0, red[wv][3]); ey0 = min(ey0, red[wv][4]); ex1 = max(ex1, red[wv][5]); ey1 = max(ey1, red[wv][6]);
    }
    int* s = stats + (size_t)n * 8;
    if (n_hi) atomicAdd(s + 0, n_hi);
    if (n_lo) atomicAdd(s + 1, n_lo);
    if (area) {
      atomicAdd(s + 2, area);
      atomicMin(s + 3, ex0); atomicMin(s + 4, ey0); atomicMax(s + 5, ex1); atomicMax(s + 6, ey1);
    }
  }
}

// largest number of source indices the taps of `n` consecutive destination indices can span (scale = in / out), with room for the f32
// rounding of the tap positions: floor((n - 1) scale) + 2 in exact arithmetic, + 1 for i1, + 2 for a rounding step at either end
inline long long amg_span(int n, int in, int out) {
  if (n == 1) return std::min(in, 2);                                 // one destination index: its two taps
  return std::min<long long>(in, (long long)(n - 1) * in / out + 5);
}

// the units tile the PH x PW plane; a unit samples at most min(band, H) rows x min(chunk, W) columns of the H x W map
inline bool amg_shape(int h, int w, int H, int W, int PH, int PW, AmgShape* sh) {
  int lg = 0;
  while ((AMG_COLS << lg) < std::min(PW, AMG_CHUNK)) ++lg;
  sh->txn_log2 = lg;
  const int chunk_w = AMG_COLS << lg;
  const long long cols = amg_span(std::min(chunk_w, W), w, W);
  int band = std::max(AMG_BAND, AMG_THREADS >> lg);
  while (band > 1 && amg_span(std::min(band, H), h, H) * cols > AMG_LDS_FLOATS) band >>= 1;
  const long long floats = amg_span(std::min(band, H), h, H) * cols;
  if (floats > AMG_LDS_FLOATS) return false;
  sh->band = band;
  sh->lds_floats = (int)floats;
  sh->nchunks = cdiv(PW, chunk_w);
  sh->nbands = cdiv(PH, band);
  return true;
}

// ---- cvmi_amg_select -----------------------------------------------------------------------------------------------------------------
// SPLIT workgroups per candidate plane.  Every workgroup evaluates the keep rule of all n_valid candidates (a few hundred integers) and
// counts the kept ones in front of its own: the slot is base + that prefix, in candidate order, whatever order the workgroups run in.  The
// running counter is read by every workgroup before it takes a ticket and written by the workgroup that takes the last one.
constexpr int SEL_THREADS = 256;
constexpr int SEL_SPLIT = 4;

// The crop the planes were decoded from, in the image: {x0, y0, x1, y1} with exclusive ends, the image's size and upstream's
// is_box_near_crop_edge tolerance.  cvmi_amg_select is the crop that is the image.
struct AmgCrop {
  int x0, y0, x1, y1, W, H, tol;
};

// upstream's is_box_near_crop_edge in integers: the box (inclusive maxima, moved to the image) has a side within tol of the crop's side
// and not within tol of the image's.  With crop = image the two tests are the same test: never true.
__device__ __forceinline__ bool amg_cut_by_crop(const int* __restrict__ s, const AmgCrop& c) {
  const int b[4] = {s[3] + c.x0, s[4] + c.y0, s[5] + c.x0, s[6] + c.y0};
  const int crop[4] = {c.x0, c.y0, c.x1, c.y1}, orig[4] = {0, 0, c.W, c.H};
  bool cut = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) cut |= abs(b[k] - crop[k]) <= c.tol && !(abs(b[k] - orig[k]) <= c.tol);
  return cut;
}

__device__ __forceinline__ bool amg_keep(const int* __restrict__ stats, const float* __restrict__ iou, int i, float iou_thresh, float stab_thresh,
                                         const AmgCrop& crop, float* stab_out) {
  const float stab = (float)stats[(size_t)i * 8 + 0] / (float)stats[(size_t)i * 8 + 1];       // 0 / 0 = NaN: fails >=
  *stab_out = stab;
  return iou[i] > iou_thresh && stab >= stab_thresh && !amg_cut_by_crop(stats + (size_t)i * 8, crop);
}

__global__ __launch_bounds__(SEL_THREADS) void amg_select_kernel(const int* __restrict__ stats, const float* __restrict__ iou,
                                                                const float* __restrict__ low, int n_valid, int ncand, int point_base,
                                                                float iou_thresh, float stab_thresh, AmgCrop crop, int P, int cap,
                                                                int* __restrict__ counter, cvmi_amg_record* __restrict__ records,
                                                                float* __restrict__ pool, float* __restrict__ nms_block) {
  __shared__ int red[SEL_THREADS / 64][2];
  __shared__ int s_before, s_total, s_base;
  const int tid = threadIdx.x, j = blockIdx.x / SEL_SPLIT, part = blockIdx.x - j * SEL_SPLIT;
  int before = 0, total = 0;
  float stab;
  for (int i = tid; i < n_valid; i += SEL_THREADS) {
    const int k = amg_keep(stats, iou, i, iou_thresh, stab_thresh, crop, &stab) ? 1 : 0;
    total += k;
    before += i < j ? k : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { before += __shfl_xor(before, off); total += __shfl_xor(total, off); }
  if ((tid & 63) == 0) { red[tid >> 6][0] = before; red[tid >> 6][1] = total; }
  __syncthreads();
  if (tid == 0) {
    int b = 0, t = 0;
    for (int wv = 0; wv < SEL_THREADS / 64; ++wv) { b += red[wv][0]; t += red[wv][1]; }
    s_before = b; s_total = t;
    s_base = __hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const long long slot = (long long)s_base + s_before;
  if (amg_keep(stats, iou, j, iou_thresh, stab_thresh, crop, &stab) && slot < cap) {
    const f32x4* src = reinterpret_cast<const f32x4*>(low + (size_t)j * P);
    f32x4* dst = reinterpret_cast<f32x4*>(pool + (size_t)slot * P);
    for (int i = part * SEL_THREADS + tid; i < P / 4; i += SEL_SPLIT * SEL_THREADS) dst[i] = src[i];
    if (part == 0 && tid == 0) {
      const int* s = stats + (size_t)j * 8;
      cvmi_amg_record r;
      r.score = iou[j]; r.stability = stab; r.area = s[2];
      r.x0 = s[3]; r.y0 = s[4]; r.x1 = s[5]; r.y1 = s[6];
      r.point = point_base + j / ncand; r.token = j - (j / ncand) * ncand; r.reserved = 0;
      records[slot] = r;
      // (cx, cy, w, h, score) for cvmi_yolo_nms: halves of integers below 2^24 are exact, so its cx - w / 2 is x0 again
      const float fx0 = (float)r.x0, fy0 = (float)r.y0, fx1 = (float)r.x1, fy1 = (float)r.y1;
      nms_block[slot] = (fx0 + fx1) / 2.f;
      nms_block[(size_t)cap + slot] = (fy0 + fy1) / 2.f;
      nms_block[(size_t)2 * cap + slot] = fx1 - fx0;
      nms_block[(size_t)3 * cap + slot] = fy1 - fy0;
      nms_block[(size_t)4 * cap + slot] = r.score;
    }
  }
  // the last workgroup through moves the counter: every other one has read it by then
  if (tid == 0) {
    __threadfence();
    const int ticket = atomicAdd(counter + 1, 1);
    if (ticket == (int)gridDim.x - 1) {
      const long long next = (long long)s_base + s_total;
      counter[0] = next > 0x7fffffffLL ? 0x7fffffff : (int)next;
      counter[1] = 0;
    }
  }
}

template <bool MASK, bool WIN>
int amg_score_launch(const float* low, int M, int h, int w, int H, int W, float lo, float mid, float hi, const AmgShape& sh, const AmgWindow& win,
                     int* stats, uint8_t* mask, hipStream_t s) {
  const dim3 grid(std::min(sh.nbands * sh.nchunks, AMG_GRID_CAP), M), block(AMG_THREADS);
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  const size_t lds = (size_t)sh.lds_floats * sizeof(float);
  if constexpr (MASK) {
    if (win.PW % 4 == 0 && ((uintptr_t)mask & 3) == 0) {
      hipLaunchKernelGGL((amg_score_kernel<true, true, WIN>), grid, block, lds, s, low, h, w, H, W, sy, sx, lo, mid, hi, sh, win, stats, mask);
      return 0;
    }
  }
  hipLaunchKernelGGL((amg_score_kernel<MASK, false, WIN>), grid, block, lds, s, low, h, w, H, W, sy, sx, lo, mid, hi, sh, win, stats, mask);
  return 0;
}

// the three launches of a scoring call: the map is the plane (cvmi_amg_score) or a window of it
template <bool WIN>
int amg_score_run(const char* who, const float* low, int M, int h, int w, int H, int W, float lo, float mid, float hi, const AmgWindow& win, int* stats,
                  uint8_t* mask_u8, hipStream_t s) {
  CVMI_CHECK(low && stats && M > 0 && M <= 65535 && h > 0 && w > 0 && H > 0 && W > 0, "%s: bad arguments", who);
  CVMI_CHECK((long long)win.PH * win.PW < (1ll << 31) && (long long)h * w < (1ll << 31), "%s: a plane of 2^31 pixels or more", who);
  AmgShape sh;
  CVMI_CHECK(amg_shape(h, w, H, W, win.PH, win.PW, &sh), "%s: the source rows of one output row (%d x %d -> %d x %d) do not fit the staging buffer", who, h, w, H, W);
  CVMI_CHECK((long long)sh.nbands * sh.nchunks < (1ll << 31), "%s: too many units", who);
  hipLaunchKernelGGL(amg_init_kernel, dim3(cdiv(M, 256)), dim3(256), 0, s, stats, M, H, W);
  if (mask_u8) amg_score_launch<true, WIN>(low, M, h, w, H, W, lo, mid, hi, sh, win, stats, mask_u8, s);
  else amg_score_launch<false, false>(low, M, h, w, H, W, lo, mid, hi, sh, win, stats, nullptr, s);
  hipLaunchKernelGGL(amg_finish_kernel, dim3(cdiv(M, 256)), dim3(256), 0, s, stats, M);
  CVMI_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int cvmi_amg_score(const float* low, int M, int h, int w, int H, int W, float lo, float mid, float hi, int* stats, uint8_t* mask_u8,
                              cvmi_stream_t stream_) {
  return amg_score_run<false>("amg_score", low, M, h, w, H, W, lo, mid, hi, AmgWindow{H, W, 0, 0}, stats, mask_u8, (hipStream_t)stream_);
}

extern "C" int cvmi_amg_score_window(const float* low, int M, int h, int w, int H, int W, float lo, float mid, float hi, int* stats,
                                     uint8_t* mask_u8, int PH, int PW, int wx0, int wy0, cvmi_stream_t stream_) {
  CVMI_CHECK(mask_u8, "amg_score_window: null pointer");
  CVMI_CHECK(H > 0 && W > 0 && PH > 0 && PW > 0 && wx0 >= 0 && wy0 >= 0 && (long long)wx0 + W <= PW && (long long)wy0 + H <= PH,
             "amg_score_window: the %d x %d window at (%d, %d) leaves the %d x %d plane", H, W, wx0, wy0, PH, PW);
  return amg_score_run<true>("amg_score_window", low, M, h, w, H, W, lo, mid, hi, AmgWindow{PH, PW, wx0, wy0}, stats, mask_u8, (hipStream_t)stream_);
}

namespace {

int amg_select_run(const char* who, const int* stats, const float* iou, const float* low, int n, int n_valid, int ncand, int point_base,
                   float iou_thresh, float stab_thresh, const AmgCrop& crop, int P, int cap, int* counter, cvmi_amg_record* records, float* pool,
                   float* nms_block, hipStream_t s) {
  CVMI_CHECK(stats && iou && low && counter && records && pool && nms_block, "%s: null pointer", who);
  CVMI_CHECK(n > 0 && n_valid >= 0 && n_valid <= n && n <= (1 << 20) && ncand > 0 && point_base >= 0 && cap > 0, "%s: bad arguments", who);
  CVMI_CHECK(P > 0 && P % 4 == 0 && ((uintptr_t)low & 15) == 0 && ((uintptr_t)pool & 15) == 0, "%s: planes must be a multiple of 4 floats, 16-byte aligned", who);
  if (n_valid == 0) return 0;
  hipLaunchKernelGGL(amg_select_kernel, dim3(n_valid * SEL_SPLIT), dim3(SEL_THREADS), 0, s, stats, iou, low, n_valid, ncand, point_base, iou_thresh,
                     stab_thresh, crop, P, cap, counter, records, pool, nms_block);
  CVMI_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int cvmi_amg_select(const int* stats, const float* iou, const float* low, int n, int n_valid, int ncand, int point_base,
                               float iou_thresh, float stab_thresh, int P, int cap, int* counter, cvmi_amg_record* records, float* pool,
                               float* nms_block, cvmi_stream_t stream_) {
  // no crop: the crop is the image, whatever its size, and the border filter is identically false
  return amg_select_run("amg_select", stats, iou, low, n, n_valid, ncand, point_base, iou_thresh, stab_thresh, AmgCrop{0, 0, 0, 0, 0, 0, 0}, P, cap,
                        counter, records, pool, nms_block, (hipStream_t)stream_);
}

extern "C" int cvmi_amg_select_crop(const int* stats, const float* iou, const float* low, int n, int n_valid, int ncand, int point_base,
                                    float iou_thresh, float stab_thresh, int P, int cap, int* counter, cvmi_amg_record* records, float* pool,
                                    float* nms_block, int cx0, int cy0, int cx1, int cy1, int W, int H, int edge_tol, cvmi_stream_t stream_) {
  CVMI_CHECK(W > 0 && H > 0 && W < (1 << 24) && H < (1 << 24) && 0 <= cx0 && cx0 < cx1 && cx1 <= W && 0 <= cy0 && cy0 < cy1 && cy1 <= H,
             "amg_select_crop: the crop [%d, %d, %d, %d] is empty or leaves the %d x %d image", cx0, cy0, cx1, cy1, W, H);
  CVMI_CHECK(edge_tol >= 0 && edge_tol < (1 << 24), "amg_select_crop: bad edge_tol");
  return amg_select_run("amg_select_crop", stats, iou, low, n, n_valid, ncand, point_base, iou_thresh, stab_thresh,
                        AmgCrop{cx0, cy0, cx1, cy1, W, H, edge_tol}, P, cap, counter, records, pool, nms_block, (hipStream_t)stream_);
}
