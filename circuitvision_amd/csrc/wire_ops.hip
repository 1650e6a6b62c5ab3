// Node-analysis front end (CircuitAnalyzer.get_node_connections, circuit_analyzer.py:1286-1370) on N u8 planes of different sizes,
// packed back to back:
//   node_empty / node_resize   the component boxes emptied (:1327-1345), then resize_image_keep_aspect's INTER_LINEAR resize (:787-809)
//   enhance                    enhance_lines (:289-311): GaussianBlur 5x5 sigma 1 -> dilate 3x3 x2 -> erode 3x3 x2 in one tiled pass, plus
//                              each plane's exact pixel sum (get_contours' cv2.mean(img) > 127 test, :398)
//   contours                   get_contours' findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) (:405): union-find labelling of the
//                              foreground (8-connected) and the background (4-connected, the frame outside the plane included), one
//                              lane per external component tracing its border with icvFetchContour's rules, count pass + scan + write.
//   node_connect               the contour x component-box loop of get_node_connections (:1380-1446): per (contour, box) the first contour
//                              point that passes is_point_near_bbox (:811-846), and contourMoments' integer Green sums for the ground choice;
//                              one workgroup per 1024-point chunk of a contour, so one long border does not serialise the launch.
// Terminal reclassification (CircuitAnalyzer.reclassify_terminals_based_on_connectivity, circuit_analyzer.py:2217-2311), the step before it:
//   segment_circuit            segment_circuit (:313-319: RGB2GRAY -> adaptiveThreshold(MEAN_C, BINARY_INV, 31, 21)) on windows of u8 RGB
//                              images, the boxes emptied (:2244-2249) and each plane's exact sum, in one tiled pass
//   contour_hits               node_connect without the broad phase and the moments: the contour x terminal-box table of :2272-2286
#include "common.hpp"

namespace {

constexpr int PLANE_MAX = 32;                 // planes per launch whose geometry travels in the kernel arguments
struct PlaneGeom {
  long long src_off[PLANE_MAX], dst_off[PLANE_MAX];
  int H[PLANE_MAX], W[PLANE_MAX], NH[PLANE_MAX], NW[PLANE_MAX], box0[PLANE_MAX], nbox[PLANE_MAX];
};

// ------------------------------------------------------------------------------------------------
// 1. node-mask preparation

__global__ __launch_bounds__(256) void node_empty_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int* __restrict__ boxes,
                                                         const PlaneGeom g) {
  const int n = blockIdx.y;
  const int H = g.H[n], W = g.W[n], b0 = g.box0[n], nb = g.nbox[n];
  const long long total = (long long)H * W;
  src += g.src_off[n];
  dst += g.src_off[n];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    bool in = false;
    for (int b = 0; b < nb && !in; ++b) {
      const int* bx = boxes + 4 * (size_t)(b0 + b);         // {xmin, ymin, xmax, ymax}, int() of the reference's values
      in = x >= bx[0] && x < bx[2] && y >= bx[1] && y < bx[3];
    }
    dst[i] = in ? (uint8_t)0 : src[i];
  }
}

// cv2.resize(m, (NW, NH)) INTER_LINEAR on one u8 channel: the letterbox's fixed-point path (lb_axis), without the pad.
__global__ __launch_bounds__(256) void node_resize_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const PlaneGeom g) {
  const int n = blockIdx.y;
  const int H = g.H[n], W = g.W[n], NH = g.NH[n], NW = g.NW[n];
  const long long total = (long long)NH * NW;
  src += g.src_off[n];
  dst += g.dst_off[n];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int oy = (int)(i / NW), ox = (int)(i - (long long)oy * NW);
    int v;
    if (NW == W && NH == H) {
      v = src[i];
    } else {
      int x0, x1, ax0, ax1, y0, y1, ay0, ay1;
      lb_axis(ox, NW, W, x0, x1, ax0, ax1);
      lb_axis(oy, NH, H, y0, y1, ay0, ay1);
      const int r0 = src[(size_t)y0 * W + x0] * ax0 + src[(size_t)y0 * W + x1] * ax1;
      const int r1 = src[(size_t)y1 * W + x0] * ax0 + src[(size_t)y1 * W + x1] * ax1;
      v = (((ay0 * (r0 >> 4)) >> 16) + ((ay1 * (r1 >> 4)) >> 16) + 2) >> 2;
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
    }
    dst[i] = (uint8_t)v;
  }
}

// ------------------------------------------------------------------------------------------------
// 2. enhance_lines, fused.  A TH x TW output tile reads a 6-pixel halo; the three stages run on LDS planes whose out-of-plane cells hold the
// value at the clamped position, which is exactly the replicated border cv2.dilate / cv2.erode see.  The blur reads the source through
// BORDER_REFLECT_101.  Blur taps: getGaussianKernelBitExact(5, 1) = {14, 63, 102, 63, 14} / 256 (test: tests/wire_ref.py derives them).
constexpr int ETW = 64, ETH = 32;
constexpr int EXW = ETW + 12, EXH = ETH + 12;        // source, halo 6
constexpr int EBW = ETW + 8, EBH = ETH + 8;          // blurred, halo 4
constexpr int EDW = ETW + 4, EDH = ETH + 4;          // dilated, halo 2

__device__ __forceinline__ int reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}
__device__ __forceinline__ int clampi(int p, int n) { return p < 0 ? 0 : (p >= n ? n - 1 : p); }

__global__ __launch_bounds__(256) void enhance_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, unsigned long long* __restrict__ sums,
                                                      const PlaneGeom g, int n0) {
  const int n = blockIdx.z;
  const int H = g.H[n], W = g.W[n];
  const int x0 = blockIdx.x * ETW, y0 = blockIdx.y * ETH;
  if (x0 >= W || y0 >= H) return;
  src += g.src_off[n];
  dst += g.src_off[n];
  __shared__ uint8_t xs[EXH][EXW];
  __shared__ int rs[EXH][EBW];                        // row pass at the blurred stage's (clamped) columns
  __shared__ uint8_t bs[EBH][EBW];
  __shared__ uint8_t dr[EBH][EDW];                    // dilate, row pass
  __shared__ uint8_t ds[EDH][EDW];
  __shared__ uint8_t er[EDH][ETW];                    // erode, row pass
  __shared__ unsigned long long red[4];
  const int tid = threadIdx.x;
  // source cell (r, c) = x[refl(y0 - 6 + r), refl(x0 - 6 + c)]
  for (int i = tid; i < EXH * EXW; i += 256) {
    const int r = i / EXW, c = i - r * EXW;
    xs[r][c] = src[(size_t)reflect101(y0 - 6 + r, H) * W + reflect101(x0 - 6 + c, W)];
  }
  __syncthreads();
  // blurred cell (r, c) = blur at (clamp(y0 - 4 + r), clamp(x0 - 4 + c)); rows of the row pass at source rows, columns at clamped columns
  for (int i = tid; i < EXH * EBW; i += 256) {
    const int r = i / EBW, c = i - r * EBW;
    const int cx = clampi(x0 - 4 + c, W) - (x0 - 6);            // source-local column of the clamped centre (2 .. EXW - 3)
    rs[r][c] = 14 * xs[r][cx - 2] + 63 * xs[r][cx - 1] + 102 * xs[r][cx] + 63 * xs[r][cx + 1] + 14 * xs[r][cx + 2];
  }
  __syncthreads();
  for (int i = tid; i < EBH * EBW; i += 256) {
    const int r = i / EBW, c = i - r * EBW;
    const int cy = clampi(y0 - 4 + r, H) - (y0 - 6);
    const int s = 14 * rs[cy - 2][c] + 63 * rs[cy - 1][c] + 102 * rs[cy][c] + 63 * rs[cy + 1][c] + 14 * rs[cy + 2][c];
    bs[r][c] = (uint8_t)((s + 32768) >> 16);
  }
  __syncthreads();
  // dilated cell (r, c) = dilated at (clamp(y0 - 2 + r), clamp(x0 - 2 + c)) = max of the blurred cells around that clamped centre
  for (int i = tid; i < EBH * EDW; i += 256) {
    const int r = i / EDW, c = i - r * EDW;
    const int cx = clampi(x0 - 2 + c, W) - (x0 - 4);
    uint8_t m = bs[r][cx - 2];
#pragma unroll
    for (int j = -1; j <= 2; ++j) m = max(m, bs[r][cx + j]);
    dr[r][c] = m;
  }
  __syncthreads();
  for (int i = tid; i < EDH * EDW; i += 256) {
    const int r = i / EDW, c = i - r * EDW;
    const int cy = clampi(y0 - 2 + r, H) - (y0 - 4);
    uint8_t m = dr[cy - 2][c];
#pragma unroll
    for (int j = -1; j <= 2; ++j) m = max(m, dr[cy + j][c]);
    ds[r][c] = m;
  }
  __syncthreads();
  for (int i = tid; i < EDH * ETW; i += 256) {
    const int r = i / ETW, c = i - r * ETW;
    const int cx = min(x0 + c, W - 1) - (x0 - 2);
    uint8_t m = ds[r][cx - 2];
#pragma unroll
    for (int j = -1; j <= 2; ++j) m = min(m, ds[r][cx + j]);
    er[r][c] = m;
  }
  __syncthreads();
  unsigned long long acc = 0;
  for (int i = tid; i < ETH * ETW; i += 256) {
    const int r = i / ETW, c = i - r * ETW;
    const int y = y0 + r, x = x0 + c;
    if (y < H && x < W) {
      const int cy = r + 2;
      uint8_t m = er[cy - 2][c];
#pragma unroll
      for (int j = -1; j <= 2; ++j) m = min(m, er[cy + j][c]);
      dst[(size_t)y * W + x] = m;
      acc += m;
    }
  }
  // exact integer plane sum: wave reduction, one 64-bit atomic per block
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) atomicAdd(sums + n0 + n, red[0] + red[1] + red[2] + red[3]);
}

// ------------------------------------------------------------------------------------------------
// 3. external contours.  Device plane table (written by contour_table_kernel from the launch arguments) so that every later kernel and
// the scans see all N planes.  Pixel p of plane n has the packed index pix + y * W + x: labels are packed indices, and the union-find
// keeps the minimum index of a set as its root -- the raster-first pixel of a component, which is where its border trace starts.
struct PlaneRec {
  long long pix;        // first pixel in the packed planes
  int H, W;
  int row0;             // first row in the packed row list (sum of H_m, m < n)
  int root0;            // first slot of the per-plane root capacity (sum of ceil(H_m / 2) * ceil(W_m / 2))
};

__global__ void contour_table_kernel(PlaneRec* tab, const PlaneGeom g, int n0, int nb, long long pix, int row0, int root0) {
  if (threadIdx.x != 0) return;
  for (int n = 0; n < nb; ++n) {
    tab[n0 + n] = PlaneRec{pix, g.H[n], g.W[n], row0, root0};
    pix += (long long)g.H[n] * g.W[n];
    row0 += g.H[n];
    root0 += ((g.H[n] + 1) / 2) * ((g.W[n] + 1) / 2);
  }
}

// foreground = non-zero, or != 255 when the plane's sum exceeds 127 * H * W (get_contours' inversion); binarize: the reference's
// img[img == 255] = 1 on the caller's array when it did not invert (:401)
__global__ __launch_bounds__(256) void label_init_kernel(uint8_t* __restrict__ planes, const unsigned long long* __restrict__ sums, const PlaneRec* tab,
                                                         int* __restrict__ lab, uint8_t* __restrict__ fgm, uint8_t* __restrict__ touch, int binarize) {
  const PlaneRec t = tab[blockIdx.y];
  const long long total = (long long)t.H * t.W;
  const bool inv = sums != nullptr && sums[blockIdx.y] > 127ull * (unsigned long long)total;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long p = t.pix + i;
    const uint8_t v = planes[p];
    fgm[p] = inv ? v != 255 : v != 0;
    if (binarize && !inv && v == 255) planes[p] = 1;
    lab[p] = (int)p;
    touch[p] = 0;
  }
}

__global__ __launch_bounds__(256) void label_merge_kernel(const PlaneRec* tab, int* __restrict__ lab, const uint8_t* __restrict__ fgm) {
  const PlaneRec t = tab[blockIdx.y];
  const long long total = (long long)t.H * t.W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int y = (int)(i / t.W), x = (int)(i - (long long)y * t.W);
    const int p = (int)(t.pix + i);
    const uint8_t f = fgm[p];
    if (x > 0 && fgm[p - 1] == f) uf_union(lab, p, p - 1);
    if (y > 0) {
      if (fgm[p - t.W] == f) uf_union(lab, p, p - t.W);
      if (f) {                                                              // 8-connected foreground: the diagonals above too
        if (x > 0 && fgm[p - t.W - 1]) uf_union(lab, p, p - t.W - 1);
        if (x + 1 < t.W && fgm[p - t.W + 1]) uf_union(lab, p, p - t.W + 1);
      }
    }
  }
}

// every pixel to its root; a background set that reaches the plane's edge touches the zero frame findContours pads the plane with
__global__ __launch_bounds__(256) void label_flatten_kernel(const PlaneRec* tab, int* __restrict__ lab, const uint8_t* __restrict__ fgm,
                                                            uint8_t* __restrict__ touch) {
  const PlaneRec t = tab[blockIdx.y];
  const long long total = (long long)t.H * t.W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int y = (int)(i / t.W), x = (int)(i - (long long)y * t.W);
    const int p = (int)(t.pix + i);
    const int r = uf_find(lab, p);
    lab[p] = r;
    if (!fgm[p] && (x == 0 || y == 0 || x == t.W - 1 || y == t.H - 1)) touch[r] = 1;
  }
}

// an external component's root: foreground, its own root, and its left neighbour (background: a foreground one would be 8-adjacent) in
// the outer background, or the frame
__device__ __forceinline__ bool is_ext_root(const int* lab, const uint8_t* fgm, const uint8_t* touch, int p, int x) {
  return fgm[p] && lab[p] == p && (x == 0 || touch[lab[p - 1]]);
}

// one wave per row: number of external roots in the row
__global__ __launch_bounds__(256) void root_count_kernel(const PlaneRec* tab, const int* __restrict__ lab, const uint8_t* __restrict__ fgm,
                                                         const uint8_t* __restrict__ touch, int* __restrict__ row_cnt) {
  const PlaneRec t = tab[blockIdx.y];
  const int y = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (y >= t.H) return;
  int c = 0;
  for (int x = lane; x < t.W; x += 64) c += is_ext_root(lab, fgm, touch, (int)(t.pix + (long long)y * t.W + x), x);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) row_cnt[t.row0 + y] = c;
}

// exclusive scan of n ints by one block of 1024 (n read from the device when n_dev is given); out[n] = the total, also copied to *total
__global__ __launch_bounds__(1024) void scan_kernel(const int* __restrict__ in, int* __restrict__ out, int n, const int* n_dev, int* total) {
  __shared__ int part[1024];
  if (n_dev) n = *n_dev;
  const int tid = threadIdx.x;
  const int per = (n + 1023) / 1024;
  const int b = min(n, tid * per), e = min(n, b + per);
  int s = 0;
  for (int i = b; i < e; ++i) s += in[i];
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - s;
  for (int i = b; i < e; ++i) {
    const int v = in[i];
    out[i] = run;
    run += v;
  }
  if (tid == 1023) {
    out[n] = part[1023];
    if (total) *total = part[1023];
  }
}

// one wave per row: the roots in raster order get forward ranks g; plane n's contours are listed in REVERSE raster order of their roots
// (findContours inserts each new contour at the head of the list), so root g lands in slot base + (cnt - 1 - (g - base))
__global__ __launch_bounds__(256) void root_assign_kernel(const PlaneRec* tab, int N, const int* __restrict__ lab, const uint8_t* __restrict__ fgm,
                                                          const uint8_t* __restrict__ touch, const int* __restrict__ row_off, int* __restrict__ roots,
                                                          int* __restrict__ counts) {
  const int n = blockIdx.y;
  const PlaneRec t = tab[n];
  const int y = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (y >= t.H) return;
  const int base = row_off[t.row0];
  const int cnt = row_off[t.row0 + t.H] - base;
  if (y == 0 && lane == 0) counts[n] = cnt;
  int g = row_off[t.row0 + y];
  for (int x0 = 0; x0 < t.W; x0 += 64) {
    const int x = x0 + lane;
    const int p = (int)(t.pix + (long long)y * t.W + x);
    const bool r = x < t.W && is_ext_root(lab, fgm, touch, p, x);
    const unsigned long long m = __ballot(r);
    if (r) {
      const int k = g + __popcll(m & ((1ull << lane) - 1ull));
      roots[2 * base + cnt - 1 - k] = p;
    }
    g += __popcll(m);
  }
}

// ---- the border trace (icvFetchContour, CHAIN_APPROX_SIMPLE) -----------------------------------------------------------------------
// direction codes s: 0 right, 1 up-right, 2 up, 3 up-left, 4 left, 5 down-left, 6 down, 7 down-right
__constant__ int8_t kDX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
__constant__ int8_t kDY[8] = {0, -1, -1, -1, 0, 1, 1, 1};

struct BitPlane {                     // the plane's foreground, one bit per pixel (LDS) or one byte per pixel (global)
  const uint32_t* bits;
  const uint8_t* bytes;
  int H, W, wpr;
  __device__ __forceinline__ bool at(int x, int y) const {
    if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H) return false;   // the zero frame
    if (bits) return (bits[y * wpr + (x >> 5)] >> (x & 31)) & 1u;
    return bytes[(size_t)y * W + x] != 0;
  }
};

struct TraceOut {
  int npts, steps, xmin, ymin, xmax, ymax;
  long long area2;                    // twice the signed shoelace area of the emitted points
};

template <bool WRITE>
__device__ TraceOut trace_border(const BitPlane& f, int x0, int y0, int* __restrict__ pts, int cap_left) {
  TraceOut o{0, 0, x0, y0, x0, y0, 0};
  int fx = x0, fy = y0, px = x0, py = y0;            // first and previous emitted point
  auto emit = [&](int x, int y) {
    if (WRITE && o.npts < cap_left) { pts[2 * o.npts] = x; pts[2 * o.npts + 1] = y; }
    if (o.npts) o.area2 += (long long)px * y - (long long)x * py;
    else { fx = x; fy = y; }
    o.xmin = min(o.xmin, x); o.xmax = max(o.xmax, x); o.ymin = min(o.ymin, y); o.ymax = max(o.ymax, y);
    px = x; py = y;
    ++o.npts;
  };
  int s = 4, x1 = x0, y1 = y0;
  do {                                                // first neighbour: s = 3, 2, 1, 0, 7, 6, 5
    s = (s - 1) & 7;
    x1 = x0 + kDX[s];
    y1 = y0 + kDY[s];
  } while (s != 4 && !f.at(x1, y1));
  if (s == 4) {                                       // a single pixel
    emit(x0, y0);
    return o;
  }
  int x3 = x0, y3 = y0, prev_s = s ^ 4;
  for (;;) {
    int x4, y4;
    for (;;) {                                        // counter-clockwise from back + 1
      ++s;
      x4 = x3 + kDX[s & 7];
      y4 = y3 + kDY[s & 7];
      if (s >= 15 || f.at(x4, y4)) break;
    }
    s &= 7;
    ++o.steps;
    if (s != prev_s) {
      emit(x3, y3);
      prev_s = s;
    }
    if (x4 == x0 && y4 == y0 && x3 == x1 && y3 == y1) break;
    x3 = x4;
    y3 = y4;
    s = (s + 4) & 7;
  }
  o.area2 += (long long)px * fy - (long long)fx * py;  // closing edge
  return o;
}

// one workgroup per plane, one lane per external contour.  Count pass (WRITE = false): npts per slot, the caller's per-contour record
// {plane, npts, -, x, y, w, h, steps} and 2 x area when the slot is within cap_contours, the longest border (steps) in counts[N + 2].
// Write pass: the points at their scanned offsets, and the offset into the record, where they fit in cap_points.
template <bool WRITE>
__global__ __launch_bounds__(256) void trace_kernel(const PlaneRec* tab, int N, const uint8_t* __restrict__ fgm, const int* __restrict__ roots,
                                                    const int* __restrict__ row_off, int* __restrict__ npts, const int* __restrict__ pt_off,
                                                    int use_lds, int cap_contours, int cap_points, int* __restrict__ counts, int* __restrict__ info,
                                                    long long* __restrict__ area2, int* __restrict__ points) {
  extern __shared__ uint32_t bits[];
  const int n = blockIdx.x;
  const PlaneRec t = tab[n];
  const int base = row_off[t.row0];
  const int cnt = row_off[t.row0 + t.H] - base;
  if (cnt == 0) return;
  const uint8_t* fp = fgm + t.pix;
  BitPlane f{nullptr, fp, t.H, t.W, (t.W + 31) >> 5};
  if (use_lds) {
    const int words = t.H * f.wpr;
    for (int w = threadIdx.x; w < words; w += blockDim.x) {
      const int y = w / f.wpr, xb = (w - y * f.wpr) * 32;
      const uint8_t* row = fp + (size_t)y * t.W;
      uint32_t v = 0;
      for (int b = 0; b < 32 && xb + b < t.W; ++b) v |= (uint32_t)(row[xb + b] != 0) << b;
      bits[w] = v;
    }
    __syncthreads();
    f.bits = bits;
  }
  int longest = 0;
  for (int k = threadIdx.x; k < cnt; k += blockDim.x) {
    const int slot = base + k;
    const int p = roots[slot];
    const int local = (int)(p - t.pix);
    const int y0 = local / t.W, x0 = local - y0 * t.W;
    if (!WRITE) {
      const TraceOut o = trace_border<false>(f, x0, y0, nullptr, 0);
      npts[slot] = o.npts;
      longest = max(longest, o.steps);
      if (slot < cap_contours) {
        int* r = info + 8 * (size_t)slot;
        r[0] = n; r[1] = o.npts; r[2] = -1;
        r[3] = o.xmin; r[4] = o.ymin; r[5] = o.xmax - o.xmin + 1; r[6] = o.ymax - o.ymin + 1; r[7] = o.steps;
        area2[slot] = o.area2;
      }
    } else {
      const int off = pt_off[slot];
      const int fit = off < cap_points ? min(npts[slot], cap_points - off) : 0;
      if (fit > 0) trace_border<true>(f, x0, y0, points + 2 * (size_t)off, fit);
      if (slot < cap_contours) info[8 * (size_t)slot + 2] = off;
    }
  }
  if (!WRITE) {
    for (int o = 32; o > 0; o >>= 1) longest = max(longest, __shfl_xor(longest, o));
    if ((threadIdx.x & 63) == 0) atomicMax(counts + N + 2, longest);
  }
}

inline int grid_for(long long total, int block = 256, int cap = 1024) {
  long long g = (total + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

constexpr size_t kLdsMax = 160 * 1024;              // LDS of one gfx950 workgroup; a dynamic request of all of it is accepted (row lds_160k_exact)

struct Workspace {
  PlaneRec* tab;
  int *lab, *row_cnt, *row_off, *roots, *npts, *pt_off;
  uint8_t *fgm, *touch;
};

// sizes of the packed geometry; false on a bad plane
bool contour_totals(int N, const int* sizes, long long& pix, long long& rows, long long& roots) {
  pix = rows = roots = 0;
  for (int n = 0; n < N; ++n) {
    const int H = sizes[2 * (size_t)n], W = sizes[2 * (size_t)n + 1];
    if (H <= 0 || W <= 0) return false;
    pix += (long long)H * W;
    rows += H;
    roots += (long long)((H + 1) / 2) * ((W + 1) / 2);
  }
  return true;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

size_t carve(void* base, int N, long long pix, long long rows, long long roots, Workspace* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { void* p = base ? (char*)base + off : nullptr; off += align256(bytes); return p; };
  Workspace t;
  t.tab = (PlaneRec*)take(sizeof(PlaneRec) * (N + 1));
  t.lab = (int*)take(4 * (size_t)pix);
  t.row_cnt = (int*)take(4 * (size_t)rows);
  t.row_off = (int*)take(4 * (size_t)(rows + 1));
  t.roots = (int*)take(4 * (size_t)roots);
  t.npts = (int*)take(4 * (size_t)roots);
  t.pt_off = (int*)take(4 * (size_t)(roots + 1));
  t.fgm = (uint8_t*)take((size_t)pix);
  t.touch = (uint8_t*)take((size_t)pix);
  if (w) *w = t;
  return off;
}

// fill the geometry table of planes [n0, n0 + nb)
void fill_geom(PlaneGeom& g, int n0, int nb, const int* sizes, int stride, long long& src_off, long long& dst_off) {
  for (int n = 0; n < PLANE_MAX; ++n) {
    if (n < nb) {
      const int* s = sizes + (size_t)stride * (n0 + n);
      g.H[n] = s[0]; g.W[n] = s[1];
      g.NH[n] = stride >= 4 ? s[2] : s[0];
      g.NW[n] = stride >= 4 ? s[3] : s[1];
      g.src_off[n] = src_off; g.dst_off[n] = dst_off;
      src_off += (long long)g.H[n] * g.W[n];
      dst_off += (long long)g.NH[n] * g.NW[n];
    } else {
      g.H[n] = g.W[n] = g.NH[n] = g.NW[n] = 1; g.src_off[n] = g.dst_off[n] = 0;
    }
    g.box0[n] = g.nbox[n] = 0;
  }
}

// ------------------------------------------------------------------------------------------------
// 4. contours x component boxes (get_node_connections :1380-1446) and contourMoments' sums.  A contour is cut into chunks of NC_CHUNK
// points, one workgroup each: wave w holds points [256 w, 256 w + 256) of the chunk, four per lane (point 64 j + lane in register j), so
// the first set bit of the first non-empty ballot is the wave's first hit in contour order.
constexpr int NC_CHUNK = 1024;                // points per workgroup
constexpr int NC_BOX_TILE = 256;              // boxes in LDS at a time
constexpr int NC_NONE = 0x7fffffff;           // `first` before any hit

__global__ __launch_bounds__(256) void node_chunks_kernel(const int* __restrict__ info, int C, int* __restrict__ nchunks) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) nchunks[c] = (max(info[8 * (size_t)c + 1], 0) + NC_CHUNK - 1) / NC_CHUNK;
}

// is_point_near_bbox (:811-846): inside the closed box, or within t of one of the four edge LINES (not of the rectangle)
__device__ __forceinline__ bool near_box(int px, int py, int xmin, int ymin, int xmax, int ymax, int t) {
  if (xmin <= px && px <= xmax && ymin <= py && py <= ymax) return true;
  const long long x = px, y = py, tt = t;
  return llabs(x - xmin) <= tt || llabs(x - xmax) <= tt || llabs(y - ymin) <= tt || llabs(y - ymax) <= tt;
}

// BROAD: the broad phase of get_node_connections; MOMENTS: contourMoments' sums.  <true, true> is cvmi_node_connect, <false, false> the
// loop of reclassify_terminals_based_on_connectivity (:2279-2286), which tests every contour against every terminal.
template <bool BROAD, bool MOMENTS>
__global__ __launch_bounds__(256) void node_connect_kernel(const int* __restrict__ info, const int* __restrict__ points, int C, int P, int N,
                                                           const int* __restrict__ boxes, const int* __restrict__ box_start,
                                                           const int* __restrict__ pair_start, const int* __restrict__ chunk_start,
                                                           int* __restrict__ first, unsigned long long* __restrict__ moments) {
  __shared__ int s_box[NC_BOX_TILE * 5];
  __shared__ int s_min[NC_BOX_TILE];
  __shared__ long long s_mom[4][3];
  const int blk = blockIdx.x;
  if (blk >= chunk_start[C]) return;
  int lo = 0, hi = C - 1;                                 // the last contour whose first chunk is <= blk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_start[mid] <= blk) lo = mid; else hi = mid - 1;
  }
  const int c = lo, k = blk - chunk_start[c];
  const int* r = info + 8 * (size_t)c;
  const int n = r[0], npts = r[1], off = r[2], rx = r[3], ry = r[4], rw = r[5], rh = r[6];
  if (n < 0 || n >= N || off < 0 || npts <= 0 || (long long)off + npts > P) return;       // a record that does not describe `points`
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int* pts = points + 2 * (size_t)off;
  int px[4], py[4];
  bool ok[4];
  long long a00 = 0, a10 = 0, a01 = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = k * NC_CHUNK + wave * 256 + j * 64 + lane;
    ok[j] = i < npts;
    px[j] = py[j] = 0;
    if (ok[j]) {
      const int ip = i ? i - 1 : npts - 1;                // the predecessor: the previous chunk's last point, or the contour's last
      px[j] = pts[2 * (size_t)i];
      py[j] = pts[2 * (size_t)i + 1];
      if (!MOMENTS) continue;
      const long long xp = pts[2 * (size_t)ip], yp = pts[2 * (size_t)ip + 1], x = px[j], y = py[j];
      const long long dxy = xp * y - x * yp;
      a00 += dxy;
      a10 += dxy * (xp + x);
      a01 += dxy * (yp + y);
    }
  }
  if (MOMENTS) {
    for (int o = 32; o > 0; o >>= 1) {
      a00 += __shfl_xor(a00, o);
      a10 += __shfl_xor(a10, o);
      a01 += __shfl_xor(a01, o);
    }
    if (lane == 0) { s_mom[wave][0] = a00; s_mom[wave][1] = a10; s_mom[wave][2] = a01; }
    __syncthreads();
    if (tid < 3)                                          // two's-complement wrap makes the unsigned add the signed sum
      atomicAdd(moments + 3 * (size_t)c + tid, (unsigned long long)(s_mom[0][tid] + s_mom[1][tid] + s_mom[2][tid] + s_mom[3][tid]));
  }

  const int b0 = box_start[n];
  const int nb = min(box_start[n + 1] - b0, pair_start[c + 1] - pair_start[c]);
  int* out = first + pair_start[c];
  for (int t0 = 0; t0 < nb; t0 += NC_BOX_TILE) {
    const int tn = min(NC_BOX_TILE, nb - t0);
    __syncthreads();                                      // the previous tile has been read
    for (int q = tid; q < tn * 5; q += 256) s_box[q] = boxes[5 * (size_t)(b0 + t0) + q];
    for (int q = tid; q < tn; q += 256) s_min[q] = NC_NONE;
    __syncthreads();
    for (int b = 0; b < tn; ++b) {
      const int xmin = s_box[5 * b], ymin = s_box[5 * b + 1], xmax = s_box[5 * b + 2], ymax = s_box[5 * b + 3], t = s_box[5 * b + 4];
      if (BROAD && (xmax < rx || xmin > rx + rw || ymax < ry || ymin > ry + rh)) continue;   // broad phase (:1399-1401), no threshold
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned long long m = __ballot(ok[j] && near_box(px[j], py[j], xmin, ymin, xmax, ymax, t));
        if (m) {                                          // wave-uniform
          if (lane == 0) atomicMin(&s_min[b], wave * 256 + j * 64 + (__ffsll((long long)m) - 1));
          break;
        }
      }
    }
    __syncthreads();
    for (int q = tid; q < tn; q += 256)
      if (s_min[q] != NC_NONE) atomicMin(out + t0 + q, k * NC_CHUNK + s_min[q]);
  }
}

__global__ __launch_bounds__(256) void node_first_finish_kernel(int* __restrict__ first, int total) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x)
    if (first[i] == NC_NONE) first[i] = -1;
}

struct ConnectSpace {
  int *box_start, *pair_start, *nchunks, *chunk_start;
};

size_t carve_connect(void* base, int N, int C, ConnectSpace* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { void* p = base ? (char*)base + off : nullptr; off += align256(bytes); return p; };
  ConnectSpace t;
  t.box_start = (int*)take(4 * ((size_t)N + 1));
  t.pair_start = (int*)take(4 * ((size_t)C + 1));
  t.nchunks = (int*)take(4 * ((size_t)C + 1));
  t.chunk_start = (int*)take(4 * ((size_t)C + 1));
  if (w) *w = t;
  return off;
}

// ------------------------------------------------------------------------------------------------
// 5. segment_circuit (:313-319) + the box emptying of reclassify_terminals_based_on_connectivity (:2244-2249), fused.  Plane n is an H x W
// window of a u8 [., ., 3] image: byte src_off, row pitch in bytes; the 31 x 31 mean replicates the WINDOW's border (clamped window
// coordinates), so nothing outside the window is read.  A 128 x 64 output tile: grey once per halo cell (halo 15) into LDS, 31-tap row sums
// by a running sum (u16: 31 * 255 = 7905), then each thread walks 32 rows of one column with a running column sum (<= 961 * 255 = 245055).
// cvRound(S / 961) = (2 S + 961) / 1922 in integers (961 is odd: no ties; tests/test_terminal_reclass_cpu.py checks all 245056 sums).
constexpr int STW = 128, STH = 64, SHALO = 15, SKS = 2 * SHALO + 1;
constexpr int SGW = STW + 2 * SHALO, SGH = STH + 2 * SHALO;      // grey cells: 158 x 94
constexpr int SGP = 160;                                          // LDS row pitch of the grey cells
constexpr int SSEG = 16;                                          // row-sum outputs per running sum
constexpr int SCOL = 32;                                          // rows per thread in the column pass: 128 columns x 2 halves = 256 threads
constexpr int SRECT_TILE = 256;                                   // rectangles in LDS at a time
static_assert(STW * (STH / SCOL) == 256 && STW % SSEG == 0 && SGP >= SGW, "segment_circuit tile");

struct SegGeom {
  long long src_off[PLANE_MAX], dst_off[PLANE_MAX];
  int pitch[PLANE_MAX], H[PLANE_MAX], W[PLANE_MAX], box0[PLANE_MAX], nbox[PLANE_MAX];
};

__global__ __launch_bounds__(256) void segment_circuit_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int* __restrict__ rects,
                                                              unsigned long long* __restrict__ sums, const SegGeom g, int n0, int red) {
  const int n = blockIdx.z;
  const int H = g.H[n], W = g.W[n];
  const int x0 = blockIdx.x * STW, y0 = blockIdx.y * STH;
  if (x0 >= W || y0 >= H) return;
  const uint8_t* sp = src + g.src_off[n];
  uint8_t* dp = dst + g.dst_off[n];
  const long long pitch = g.pitch[n];
  __shared__ uint8_t gs[SGH][SGP];
  __shared__ uint16_t rs[SGH][STW];
  __shared__ int s_rect[SRECT_TILE * 4];
  __shared__ unsigned long long part[4];
  const int tid = threadIdx.x;
  const int tw = min(STW, W - x0), th = min(STH, H - y0);       // the part of the tile inside the plane
  const int gw = tw + 2 * SHALO, gh = th + 2 * SHALO;
  // grey cell (r, c) = grey at (clamp(y0 - 15 + r), clamp(x0 - 15 + c)): RGB2Gray<uchar>, red on channel `red`, blue on 2 - red
  for (int i = tid; i < gh * gw; i += 256) {
    const int r = i / gw, c = i - r * gw;
    const uint8_t* p = sp + clampi(y0 - SHALO + r, H) * pitch + 3 * clampi(x0 - SHALO + c, W);
    gs[r][c] = (uint8_t)((p[red] * 9798 + p[1] * 19235 + p[2 - red] * 3735 + 16384) >> 15);
  }
  __syncthreads();
  // rs[r][c] = gs[r][c .. c + 30]: one running sum per SSEG outputs (cells past gw are never-used outputs' inputs)
  const int nseg = (tw + SSEG - 1) / SSEG;
  for (int i = tid; i < gh * nseg; i += 256) {
    const int r = i / nseg, c0 = (i - r * nseg) * SSEG;
    int s = 0;
#pragma unroll
    for (int k = 0; k < SKS; ++k) s += gs[r][c0 + k];
    rs[r][c0] = (uint16_t)s;
#pragma unroll
    for (int j = 1; j < SSEG; ++j) {
      s += gs[r][c0 + j + SKS - 1] - gs[r][c0 + j - 1];
      rs[r][c0 + j] = (uint16_t)s;
    }
  }
  __syncthreads();
  // the rectangles that empty: bit j of `kill` = pixel (x0 + c, y0 + rb + j) lies in one of them
  const int c = tid & (STW - 1), rb = (tid >> 7) * SCOL;
  const int b0 = g.box0[n], nb = g.nbox[n];
  uint32_t kill = 0;
  for (int t0 = 0; t0 < nb; t0 += SRECT_TILE) {
    const int tn = min(SRECT_TILE, nb - t0);
    if (t0) __syncthreads();                                     // the previous tile has been read
    for (int q = tid; q < tn * 4; q += 256) s_rect[q] = rects[4 * (size_t)(b0 + t0) + q];
    __syncthreads();
    for (int b = 0; b < tn; ++b) {
      const int rx0 = s_rect[4 * b], ry0 = s_rect[4 * b + 1], rx1 = s_rect[4 * b + 2], ry1 = s_rect[4 * b + 3];   // [x0, x1) x [y0, y1)
      if (rx1 <= x0 || rx0 >= x0 + STW || ry1 <= y0 || ry0 >= y0 + STH) continue;                                  // block-uniform
      if (x0 + c >= rx0 && x0 + c < rx1) {
        const int lo = max(ry0 - (y0 + rb), 0), hi = min(ry1 - (y0 + rb), SCOL);
        if (lo < hi) kill |= (hi - lo == 32 ? 0xffffffffu : ((1u << (hi - lo)) - 1u)) << lo;
      }
    }
  }
  unsigned cnt = 0;
  if (c < tw && rb < th) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < SKS; ++k) s += rs[rb + k][c];
    const int rows = min(SCOL, th - rb);
    for (int j = 0; j < rows; ++j) {
      if (j) s += rs[rb + j + SKS - 1][c] - rs[rb + j - 1][c];
      const int mean = (2 * s + SKS * SKS) / (2 * SKS * SKS);
      const bool on = (int)gs[rb + j + SHALO][c + SHALO] - mean <= -21 && !((kill >> j) & 1u);     // THRESH_BINARY_INV, delta 21
      dp[(size_t)(y0 + rb + j) * W + x0 + c] = on ? (uint8_t)255 : (uint8_t)0;
      cnt += on;
    }
  }
  // exact integer plane sum: wave reduction, one 64-bit atomic per block
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((tid & 63) == 0) part[tid >> 6] = 255ull * cnt;
  __syncthreads();
  if (tid == 0) atomicAdd(sums + n0 + n, part[0] + part[1] + part[2] + part[3]);
}

}  // namespace

extern "C" int cvmi_node_prepare(const uint8_t* src, int N, const int* sizes, const int* boxes, const int* box_start, uint8_t* emptied,
                                 uint8_t* resized, cvmi_stream_t stream_) {
  CVMI_CHECK(src && sizes && box_start && emptied && resized && N > 0, "node_prepare: bad arguments");
  CVMI_CHECK(emptied != src, "node_prepare: emptied must not alias src");
  CVMI_CHECK(box_start[0] == 0 && (box_start[N] == 0 || boxes), "node_prepare: bad box offsets");
  for (int n = 0; n < N; ++n) {
    const int* s = sizes + 4 * (size_t)n;
    CVMI_CHECK(s[0] > 0 && s[1] > 0 && s[2] > 0 && s[3] > 0 && (long long)s[0] * s[1] < (1ll << 31) && (long long)s[2] * s[3] < (1ll << 31),
               "node_prepare: plane %d has size %d x %d -> %d x %d", n, s[0], s[1], s[2], s[3]);
    CVMI_CHECK(box_start[n + 1] >= box_start[n], "node_prepare: box offsets of plane %d decrease", n);
  }
  hipStream_t s = (hipStream_t)stream_;
  long long so = 0, dso = 0;
  for (int n0 = 0; n0 < N; n0 += PLANE_MAX) {
    const int nb = N - n0 < PLANE_MAX ? N - n0 : PLANE_MAX;
    PlaneGeom g;
    const long long so0 = so, dso0 = dso;
    long long rel_s = 0, rel_d = 0, maxs = 1, maxd = 1;
    fill_geom(g, n0, nb, sizes, 4, rel_s, rel_d);
    for (int n = 0; n < nb; ++n) {
      g.box0[n] = box_start[n0 + n];
      g.nbox[n] = box_start[n0 + n + 1] - box_start[n0 + n];
      maxs = std::max(maxs, (long long)g.H[n] * g.W[n]);
      maxd = std::max(maxd, (long long)g.NH[n] * g.NW[n]);
    }
    hipLaunchKernelGGL(node_empty_kernel, dim3(grid_for(maxs), nb), dim3(256), 0, s, src + so0, emptied + so0, boxes, g);
    hipLaunchKernelGGL(node_resize_kernel, dim3(grid_for(maxd), nb), dim3(256), 0, s, emptied + so0, resized + dso0, g);
    CVMI_LAUNCH_CHECK();
    so += rel_s;
    dso += rel_d;
  }
  return 0;
}

extern "C" int cvmi_enhance_lines(const uint8_t* src, int N, const int* sizes, uint8_t* dst, unsigned long long* sums, cvmi_stream_t stream_) {
  CVMI_CHECK(src && dst && sizes && sums && N > 0, "enhance_lines: bad arguments");
  CVMI_CHECK(src != dst, "enhance_lines: dst must not alias src");
  hipStream_t s = (hipStream_t)stream_;
  CVMI_HIP(hipMemsetAsync(sums, 0, sizeof(unsigned long long) * N, s));
  long long off = 0;
  for (int n0 = 0; n0 < N; n0 += PLANE_MAX) {
    const int nb = N - n0 < PLANE_MAX ? N - n0 : PLANE_MAX;
    PlaneGeom g;
    long long rel = 0, rel2 = 0;
    int mh = 1, mw = 1;
    fill_geom(g, n0, nb, sizes, 2, rel, rel2);
    for (int n = 0; n < nb; ++n) {
      CVMI_CHECK(g.H[n] > 0 && g.W[n] > 0 && (long long)g.H[n] * g.W[n] < (1ll << 31), "enhance_lines: plane %d has size %d x %d", n0 + n, g.H[n], g.W[n]);
      mh = std::max(mh, g.H[n]);
      mw = std::max(mw, g.W[n]);
    }
    hipLaunchKernelGGL(enhance_kernel, dim3(cdiv(mw, ETW), cdiv(mh, ETH), nb), dim3(256), 0, s, src + off, dst + off, sums, g, n0);
    CVMI_LAUNCH_CHECK();
    off += rel;
  }
  return 0;
}

extern "C" size_t cvmi_contours_workspace(int N, const int* sizes) {
  long long pix, rows, roots;
  if (N <= 0 || !sizes || !contour_totals(N, sizes, pix, rows, roots)) return 0;
  return carve(nullptr, N, pix, rows, roots, nullptr);
}

extern "C" int cvmi_external_contours(uint8_t* planes, const unsigned long long* sums, int N, const int* sizes, int binarize, void* workspace,
                                      size_t workspace_bytes, int cap_contours, int cap_points, int* counts, int* info, long long* area2,
                                      int* points, cvmi_stream_t stream_) {
  CVMI_CHECK(planes && sizes && workspace && counts && N > 0 && N <= 65535, "external_contours: bad arguments");
  CVMI_CHECK(cap_contours >= 0 && cap_points >= 0 && (cap_contours == 0 || (info && area2)) && (cap_points == 0 || points),
             "external_contours: bad output capacities");
  long long pix, rows, roots;
  CVMI_CHECK(contour_totals(N, sizes, pix, rows, roots), "external_contours: a plane has a non-positive size");
  CVMI_CHECK(pix < (1ll << 31) && roots < (1ll << 30), "external_contours: %lld pixels exceed the int32 labels", pix);
  Workspace w;
  CVMI_CHECK(carve(workspace, N, pix, rows, roots, &w) <= workspace_bytes, "external_contours: workspace of %zu bytes is short (cvmi_contours_workspace)",
             workspace_bytes);
  hipStream_t s = (hipStream_t)stream_;
  int mh = 1, maxwords = 0;
  long long maxhw = 1, p0 = 0;
  int r0 = 0, q0 = 0;
  for (int n0 = 0; n0 < N; n0 += PLANE_MAX) {
    const int nb = N - n0 < PLANE_MAX ? N - n0 : PLANE_MAX;
    PlaneGeom g;
    long long rel = 0, rel2 = 0;
    fill_geom(g, n0, nb, sizes, 2, rel, rel2);
    hipLaunchKernelGGL(contour_table_kernel, dim3(1), dim3(64), 0, s, w.tab, g, n0, nb, p0, r0, q0);
    for (int n = 0; n < nb; ++n) {
      p0 += (long long)g.H[n] * g.W[n];
      r0 += g.H[n];
      q0 += ((g.H[n] + 1) / 2) * ((g.W[n] + 1) / 2);
      mh = std::max(mh, g.H[n]);
      maxhw = std::max(maxhw, (long long)g.H[n] * g.W[n]);
      maxwords = std::max(maxwords, g.H[n] * ((g.W[n] + 31) / 32));
    }
  }
  CVMI_HIP(hipMemsetAsync(counts, 0, sizeof(int) * (N + 3), s));
  const dim3 gp(grid_for(maxhw), N), b256(256), grow(cdiv(mh, 4), N);
  hipLaunchKernelGGL(label_init_kernel, gp, b256, 0, s, planes, sums, w.tab, w.lab, w.fgm, w.touch, binarize);
  hipLaunchKernelGGL(label_merge_kernel, gp, b256, 0, s, w.tab, w.lab, w.fgm);
  hipLaunchKernelGGL(label_flatten_kernel, gp, b256, 0, s, w.tab, w.lab, w.fgm, w.touch);
  hipLaunchKernelGGL(root_count_kernel, grow, b256, 0, s, w.tab, w.lab, w.fgm, w.touch, w.row_cnt);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, w.row_cnt, w.row_off, (int)rows, nullptr, counts + N);
  hipLaunchKernelGGL(root_assign_kernel, grow, b256, 0, s, w.tab, N, w.lab, w.fgm, w.touch, w.row_off, w.roots, counts);
  const size_t lds = (size_t)maxwords * 4;
  const int use_lds = lds <= kLdsMax;
  const size_t dyn = use_lds ? lds : 0;
  if (dyn > 64 * 1024) {
    CVMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&trace_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    CVMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&trace_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
  }
  // which of the two plane forms the trace reads, and the dynamic LDS it asks for (cvmi_last_kernel)
  cvmi_note_kernel(use_lds ? "trace_kernel<lds, %d>" : "trace_kernel<global, %d>", (int)dyn);
  hipLaunchKernelGGL(trace_kernel<false>, dim3(N), b256, dyn, s, w.tab, N, w.fgm, w.roots, w.row_off, w.npts, w.pt_off, use_lds, cap_contours,
                     cap_points, counts, info, area2, points);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, w.npts, w.pt_off, 0, counts + N, counts + N + 1);
  hipLaunchKernelGGL(trace_kernel<true>, dim3(N), b256, dyn, s, w.tab, N, w.fgm, w.roots, w.row_off, w.npts, w.pt_off, use_lds, cap_contours,
                     cap_points, counts, info, area2, points);
  CVMI_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t cvmi_node_connect_workspace(int N, int C) {
  if (N <= 0 || C < 0) return 0;
  return carve_connect(nullptr, N, C, nullptr);
}

extern "C" int cvmi_node_connect(const int* info, const int* points, int C, int P, const int* boxes, int N, const int* box_start,
                                 const int* pair_start, void* workspace, size_t workspace_bytes, int* first, long long* moments,
                                 cvmi_stream_t stream_) {
  CVMI_CHECK(N > 0 && C >= 0 && P >= 0 && box_start && pair_start, "node_connect: bad arguments");
  CVMI_CHECK(box_start[0] == 0 && pair_start[0] == 0, "node_connect: offsets must start at 0");
  for (int n = 0; n < N; ++n) CVMI_CHECK(box_start[n + 1] >= box_start[n], "node_connect: box offsets of plane %d decrease", n);
  for (int c = 0; c < C; ++c) CVMI_CHECK(pair_start[c + 1] >= pair_start[c], "node_connect: pair offsets of contour %d decrease", c);
  if (C == 0) return 0;
  const int pairs = pair_start[C];
  CVMI_CHECK(info && points && moments && workspace && (box_start[N] == 0 || boxes) && (pairs == 0 || first), "node_connect: bad arguments");
  ConnectSpace w;
  CVMI_CHECK(carve_connect(workspace, N, C, &w) <= workspace_bytes, "node_connect: workspace of %zu bytes is short (cvmi_node_connect_workspace)",
             workspace_bytes);
  hipStream_t s = (hipStream_t)stream_;
  CVMI_HIP(hipMemcpyAsync(w.box_start, box_start, 4 * ((size_t)N + 1), hipMemcpyHostToDevice, s));
  CVMI_HIP(hipMemcpyAsync(w.pair_start, pair_start, 4 * ((size_t)C + 1), hipMemcpyHostToDevice, s));
  CVMI_HIP(hipMemsetAsync(moments, 0, sizeof(long long) * 3 * (size_t)C, s));
  if (pairs) CVMI_HIP(hipMemsetD32Async((hipDeviceptr_t)first, NC_NONE, (size_t)pairs, s));
  hipLaunchKernelGGL(node_chunks_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, info, C, w.nchunks);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, w.nchunks, w.chunk_start, C, nullptr, nullptr);
  const int grid = P / NC_CHUNK + C;                     // >= the sum over the contours of ceil(npts / NC_CHUNK); the rest exit at once
  hipLaunchKernelGGL((node_connect_kernel<true, true>), dim3(grid), dim3(256), 0, s, info, points, C, P, N, boxes, w.box_start, w.pair_start,
                     w.chunk_start, first, (unsigned long long*)moments);
  if (pairs) hipLaunchKernelGGL(node_first_finish_kernel, dim3(grid_for(pairs)), dim3(256), 0, s, first, pairs);
  CVMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int cvmi_segment_circuit(const uint8_t* src, size_t src_bytes, int N, const long long* planes, int red_channel, const int* rects,
                                    const int* box_start, uint8_t* dst, unsigned long long* sums, cvmi_stream_t stream_) {
  CVMI_CHECK(src && planes && box_start && dst && sums && N > 0, "segment_circuit: bad arguments");
  CVMI_CHECK(red_channel == 0 || red_channel == 2, "segment_circuit: red_channel is %d, not 0 or 2", red_channel);
  CVMI_CHECK(box_start[0] == 0, "segment_circuit: box offsets must start at 0");
  long long out = 0;
  for (int n = 0; n < N; ++n) {
    const long long *p = planes + 4 * (size_t)n, off = p[0], pitch = p[1], H = p[2], W = p[3];
    CVMI_CHECK(H > 0 && W > 0 && H * W < (1ll << 31) && pitch >= 3 * W && pitch < (1ll << 31), "segment_circuit: plane %d is %lld x %lld with pitch %lld", n,
               H, W, pitch);
    CVMI_CHECK(off >= 0 && (unsigned long long)(off + (H - 1) * pitch + 3 * W) <= src_bytes, "segment_circuit: plane %d leaves the %zu source bytes", n,
               src_bytes);
    CVMI_CHECK(box_start[n + 1] >= box_start[n], "segment_circuit: box offsets of plane %d decrease", n);
    out += H * W;
  }
  CVMI_CHECK(box_start[N] == 0 || rects, "segment_circuit: rectangles missing");
  CVMI_CHECK(dst + out <= src || src + src_bytes <= dst, "segment_circuit: dst overlaps src");
  hipStream_t s = (hipStream_t)stream_;
  CVMI_HIP(hipMemsetAsync(sums, 0, sizeof(unsigned long long) * N, s));
  long long doff = 0;
  for (int n0 = 0; n0 < N; n0 += PLANE_MAX) {
    const int nb = N - n0 < PLANE_MAX ? N - n0 : PLANE_MAX;
    SegGeom g;
    int mh = 1, mw = 1;
    for (int n = 0; n < PLANE_MAX; ++n) {
      const long long* p = planes + 4 * (size_t)(n0 + (n < nb ? n : 0));
      g.src_off[n] = p[0]; g.pitch[n] = (int)p[1]; g.H[n] = n < nb ? (int)p[2] : 0; g.W[n] = n < nb ? (int)p[3] : 0;
      g.dst_off[n] = doff;
      g.box0[n] = n < nb ? box_start[n0 + n] : 0;
      g.nbox[n] = n < nb ? box_start[n0 + n + 1] - box_start[n0 + n] : 0;
      if (n < nb) {
        doff += p[2] * p[3];
        mh = std::max(mh, g.H[n]);
        mw = std::max(mw, g.W[n]);
      }
    }
    hipLaunchKernelGGL(segment_circuit_kernel, dim3(cdiv(mw, STW), cdiv(mh, STH), nb), dim3(256), 0, s, src, dst, rects, sums, g, n0, red_channel);
    CVMI_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" size_t cvmi_contour_hits_workspace(int N, int C) { return cvmi_node_connect_workspace(N, C); }

extern "C" int cvmi_contour_hits(const int* info, const int* points, int C, int P, const int* boxes, int N, const int* box_start,
                                 const int* pair_start, void* workspace, size_t workspace_bytes, int* first, cvmi_stream_t stream_) {
  CVMI_CHECK(N > 0 && C >= 0 && P >= 0 && box_start && pair_start, "contour_hits: bad arguments");
  CVMI_CHECK(box_start[0] == 0 && pair_start[0] == 0, "contour_hits: offsets must start at 0");
  for (int n = 0; n < N; ++n) CVMI_CHECK(box_start[n + 1] >= box_start[n], "contour_hits: box offsets of plane %d decrease", n);
  for (int c = 0; c < C; ++c) CVMI_CHECK(pair_start[c + 1] >= pair_start[c], "contour_hits: pair offsets of contour %d decrease", c);
  if (C == 0 || pair_start[C] == 0) return 0;
  const int pairs = pair_start[C];
  CVMI_CHECK(info && points && workspace && boxes && first, "contour_hits: bad arguments");
  ConnectSpace w;
  CVMI_CHECK(carve_connect(workspace, N, C, &w) <= workspace_bytes, "contour_hits: workspace of %zu bytes is short (cvmi_contour_hits_workspace)",
             workspace_bytes);
  hipStream_t s = (hipStream_t)stream_;
  CVMI_HIP(hipMemcpyAsync(w.box_start, box_start, 4 * ((size_t)N + 1), hipMemcpyHostToDevice, s));
  CVMI_HIP(hipMemcpyAsync(w.pair_start, pair_start, 4 * ((size_t)C + 1), hipMemcpyHostToDevice, s));
  CVMI_HIP(hipMemsetD32Async((hipDeviceptr_t)first, NC_NONE, (size_t)pairs, s));
  hipLaunchKernelGGL(node_chunks_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, info, C, w.nchunks);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, w.nchunks, w.chunk_start, C, nullptr, nullptr);
  const int grid = P / NC_CHUNK + C;
  hipLaunchKernelGGL((node_connect_kernel<false, false>), dim3(grid), dim3(256), 0, s, info, points, C, P, N, boxes, w.box_start, w.pair_start,
                     w.chunk_start, first, (unsigned long long*)nullptr);
  hipLaunchKernelGGL(node_first_finish_kernel, dim3(grid_for(pairs)), dim3(256), 0, s, first, pairs);
  CVMI_LAUNCH_CHECK();
  return 0;
}
