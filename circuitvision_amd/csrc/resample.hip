// The resampling family: the antialiased input transform (SAM2Transforms.__call__) in its five forms, the bilinear mask return in its four,
// and the extent of a binary mask.  ONE transform body (sam2_transform_window) and ONE mask-return body (bilinear_plane); the forms differ
// only in how a launch finds its window or its plane.  Built once: every kernel computes in f32 and only a transform's last conversion depends
// on the output type, so the three output types are instances of this one translation unit (no dual-built entry point, no second build for bf16).
#include "common.hpp"
#include "bilinear.hpp"

namespace {

inline int grid_for(long long total, int block = 256, int cap = 256 * 16) {
  long long g = (total + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// threads per workgroup of every grid-stride kernel below (grid_for's default block).  A constant in the index arithmetic: a body that is inlined
// into its kernel would otherwise load blockDim through the general path (a vector load and a wait at the head of every wave).
constexpr int BLOCK = 256;

// tables that travel by value in the kernel arguments (<= 64 images / planes per launch)
constexpr int RECT_MAX = 64;
struct RectTable { int4 r[RECT_MAX]; };

// ---- SAM2Transforms.__call__: /255, antialiased bilinear (torch _upsample_bilinear2d_aa), normalise -----------
constexpr int AA_MAXTAPS = 24;
__device__ __forceinline__ void aa_axis(int i, float scale, int in, int& xmin, int& xsize, float* wt) {
  const float support = scale >= 1.f ? scale : 1.f;
  const float invscale = scale >= 1.f ? 1.f / scale : 1.f;
  const float center = scale * ((float)i + 0.5f);
  xmin = max((int)(center - support + 0.5f), 0);
  xsize = min((int)(center + support + 0.5f), in) - xmin;
  if (xsize > AA_MAXTAPS) xsize = AA_MAXTAPS;
  float total = 0.f;
  for (int j = 0; j < xsize; ++j) {
    float t = ((float)(j + xmin) - center + 0.5f) * invscale;
    t = fabsf(t);
    const float wv = t < 1.f ? 1.f - t : 0.f;
    wt[j] = wv;
    total += wv;
  }
  const float ws = total != 0.f ? 1.f / total : 0.f;
  for (int j = 0; j < xsize; ++j) wt[j] *= ws;
}

// Image blockIdx.y of the launch = the rectangle rc = {x0, y0, w, h} of the W-wide source image at src + blockIdx.y * image_stride: the crop
// between the two stages (circuit_analyzer.py:937-1284 as called at analysis_pipeline.py:177) without a cropped copy.  The resize sees nothing
// outside the window, so every form below is this arithmetic on a contiguous copy of its window.  sy = (float)h / (float)R, sx = (float)w /
// (float)R: one correctly rounded division each, on the host where the host knows the window and here (window_scales) where it does not.
template <typename T>
__device__ __forceinline__ void sam2_transform_window(const uint8_t* __restrict__ src, long long image_stride, int W, const int4 rc, float sy, float sx,
                                                      T* __restrict__ dst, int R, int swap_rb) {
  const int H0 = rc.w, W0 = rc.z;                         // the window's height, width
  src += (size_t)blockIdx.y * image_stride + ((size_t)rc.y * W + rc.x) * 3;
  dst += (size_t)blockIdx.y * R * R * 3;
  const int c0 = swap_rb ? 2 : 0, c2 = swap_rb ? 0 : 2;   // swap_rb: output channel c reads source channel 2 - c (the caller's cv2.COLOR_BGR2RGB)
  const int total = R * R;
  for (int idx = blockIdx.x * BLOCK + threadIdx.x; idx < total; idx += gridDim.x * BLOCK) {
    const int oy = idx / R, ox = idx - oy * R;
    int ymin, ysize, xmin, xsize;
    float wy[AA_MAXTAPS], wx[AA_MAXTAPS];
    aa_axis(oy, sy, H0, ymin, ysize, wy);
    aa_axis(ox, sx, W0, xmin, xsize, wx);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < ysize; ++j) {
      float row[3] = {0.f, 0.f, 0.f};
      const uint8_t* sp = src + ((size_t)(ymin + j) * W + xmin) * 3;
      for (int i = 0; i < xsize; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) row[c] += wx[i] * ((float)sp[i * 3 + (c == 0 ? c0 : c == 2 ? c2 : 1)] / 255.0f);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += wy[j] * row[c];
    }
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[(size_t)idx * 3 + c] = (T)((acc[c] - mean[c]) / stdv[c]);
  }
}

template <typename T>
__device__ __forceinline__ void sam2_transform_window(const uint8_t* __restrict__ src, long long image_stride, int W, const int4 rc, T* __restrict__ dst,
                                                      int R, int swap_rb) {
  sam2_transform_window<T>(src, image_stride, W, rc, (float)rc.w / (float)R, (float)rc.z / (float)R, dst, R, swap_rb);
}

// Four ways to find the window.  Equally sized sources: the whole image (and its scales from the host, one division per launch, not per thread).
template <typename T>
__global__ __launch_bounds__(BLOCK) void sam2_transform_kernel(T* __restrict__ dst, int R, int swap_rb, const uint8_t* __restrict__ src, int H, int W,
                                                            float sy, float sx) {
  sam2_transform_window<T>(src, (long long)H * W * 3, W, make_int4(0, 0, W, H), sy, sx, dst, R, swap_rb);
}

// A table of windows in the kernel arguments.
template <typename T>
__global__ __launch_bounds__(BLOCK) void sam2_transform_rects_kernel(T* __restrict__ dst, int R, int swap_rb, const uint8_t* __restrict__ src,
                                                                  long long image_stride, int W, const RectTable win) {
  sam2_transform_window<T>(src, image_stride, W, win.r[blockIdx.y], dst, R, swap_rb);
}

// The window table in DEVICE memory (cvmi_stage2_crop's output): nothing of the launch depends on a value the host has seen.  A window is
// clipped to the H x W image here, whatever the table holds.
template <typename T>
__global__ __launch_bounds__(BLOCK) void sam2_transform_rects_dev_kernel(T* __restrict__ dst, int R, int swap_rb, const uint8_t* __restrict__ src,
                                                                      long long image_stride, int H, int W, const int4* __restrict__ win) {
  int4 rc = win[blockIdx.y];
  rc.x = min(max(rc.x, 0), W - 1); rc.y = min(max(rc.y, 0), H - 1);
  rc.z = min(max(rc.z, 1), W - rc.x); rc.w = min(max(rc.w, 1), H - rc.y);
  sam2_transform_window<T>(src, image_stride, W, rc, dst, R, swap_rb);
}

// Sources of DIFFERENT sizes in one packed u8 buffer: image blockIdx.y is the window {x0, y0, w, h} of the row's H x W image at
// src + src_byte_offset (any byte offset: the taps are read byte by byte).
struct SrcTable { cvmi_sam2_src_row r[RECT_MAX]; };
template <typename T>
__global__ __launch_bounds__(BLOCK) void sam2_transform_srcs_kernel(T* __restrict__ dst, int R, int swap_rb, const uint8_t* __restrict__ src,
                                                                 const SrcTable tab) {
  const cvmi_sam2_src_row g = tab.r[blockIdx.y];
  sam2_transform_window<T>(src + g.src_byte_offset, 0, g.W, make_int4(g.x0, g.y0, g.w, g.h), dst, R, swap_rb);
}

// The launcher: `kernel` for the output type the caller names, on `grid` x BLOCK threads; every transform kernel takes (dst, ...) first.
#define LAUNCH_TRANSFORM(kernel, grid, stream, dst_dtype, dst, ...)                                                              \
  do {                                                                                                                           \
    if ((dst_dtype) == CVMI_F16) hipLaunchKernelGGL(kernel<_Float16>, grid, dim3(BLOCK), 0, stream, (_Float16*)(dst), __VA_ARGS__); \
    else if ((dst_dtype) == CVMI_BF16) hipLaunchKernelGGL(kernel<__bf16>, grid, dim3(BLOCK), 0, stream, (__bf16*)(dst), __VA_ARGS__); \
    else hipLaunchKernelGGL(kernel<float>, grid, dim3(BLOCK), 0, stream, (float*)(dst), __VA_ARGS__);                               \
    CVMI_LAUNCH_CHECK();                                                                                                         \
  } while (0)

inline bool is_out_type(int dt) { return dt == CVMI_F16 || dt == CVMI_BF16 || dt == CVMI_F32; }
inline size_t out_bytes(int dt) { return dt == CVMI_F32 ? 4 : 2; }

// aa_axis keeps AA_MAXTAPS taps per axis: h x w source pixels may go to R x R if 2 * max(scale, 1) + 2 taps fit on both axes
inline bool taps_fit(int h, int w, int R) {
  const float sy = (float)h / (float)R, sx = (float)w / (float)R;
  return 2.f * (sy > 1.f ? sy : 1.f) + 2.f <= AA_MAXTAPS && 2.f * (sx > 1.f ? sx : 1.f) + 2.f <= AA_MAXTAPS;
}
inline bool window_inside(int x0, int y0, int w, int h, int W, int H) {
  return x0 >= 0 && y0 >= 0 && w > 0 && h > 0 && (long long)x0 + w <= W && (long long)y0 + h <= H;
}

// ---- extent of a binary mask: min / max x, y over the non-zero pixels of each plane ----------------------------------
// (circuit_analyzer.py:364-370: cv2.findContours(EXTERNAL) + boundingRect over all contour points == the bounding
// rectangle of the non-zero pixels).  ext[0..3] starts as {W, H, -1, -1} (extent_init_kernel); every wave folds its lanes' boxes into it.
__device__ __forceinline__ void extent_fold(int* __restrict__ ext, int x0, int y0, int x1, int y1) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    x0 = min(x0, __shfl_xor(x0, off)); y0 = min(y0, __shfl_xor(y0, off));
    x1 = max(x1, __shfl_xor(x1, off)); y1 = max(y1, __shfl_xor(y1, off));
  }
  if ((threadIdx.x & 63) == 0 && x1 >= 0) {
    atomicMin(ext + 0, x0); atomicMin(ext + 1, y0);
    atomicMax(ext + 2, x1); atomicMax(ext + 3, y1);
  }
}

__global__ __launch_bounds__(BLOCK) void mask_extent_kernel(const uint8_t* __restrict__ m, int H, int W, int* __restrict__ ext) {
  const int n = blockIdx.y;
  const uint8_t* pl = m + (size_t)n * H * W;
  int x0 = W, y0 = H, x1 = -1, y1 = -1;
  const long long total = (long long)H * W;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * BLOCK) {
    if (pl[i]) {
      const int y = (int)(i / W), x = (int)(i - (long long)y * W);
      x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
    }
  }
  extent_fold(ext + n * 4, x0, y0, x1, y1);
}

// ---- the mask return: bilinear, align_corners = False (bilinear.hpp), threshold, u8, extent ------------------------------------------
// Where plane n of a launch goes and how large it is, the three ways a caller states it: plane(n, H, W) -> its first byte (or null);
// scales(h, w, H, W, sy, sx) -> the source steps (float)h / (float)H, (float)w / (float)W of an h x w source.
__device__ __forceinline__ void plane_scales(int h, int w, int H, int W, float& sy, float& sx) { sy = (float)h / (float)H; sx = (float)w / (float)W; }
struct EqualPlanes {                                      // N planes of one size, back to back; the host knows the size, so it divides (once)
  uint8_t* mask; int H, W; float sy, sx;
  EqualPlanes(uint8_t* mask, int h, int w, int H, int W) : mask(mask), H(H), W(W), sy((float)h / (float)H), sx((float)w / (float)W) {}
  __device__ __forceinline__ uint8_t* plane(int n, int& h, int& w) const { h = H; w = W; return mask ? mask + (size_t)n * H * W : nullptr; }
  __device__ __forceinline__ void scales(int, int, int, int, float& y, float& x) const { y = sy; x = sx; }
};
struct SizedPlanes {                                      // planes of DIFFERENT sizes (each image's own crop window), packed back to back:
  uint8_t* mask; RectTable sz;                            // sz.r[n] = {H, W, low and high word of the byte offset the host laid out}
  __device__ __forceinline__ uint8_t* plane(int n, int& h, int& w) const {
    h = sz.r[n].x; w = sz.r[n].y;
    return mask + (((long long)(unsigned)sz.r[n].w << 32) | (unsigned)sz.r[n].z);
  }
  __device__ __forceinline__ void scales(int h, int w, int H, int W, float& y, float& x) const { plane_scales(h, w, H, W, y, x); }
};
struct WindowPlanes {                                     // the sizes in DEVICE memory: plane n returns to the {w, h} of win[n] = {x0, y0, w, h} at
  uint8_t* mask; const int4* win; long long stride;       // mask + n * stride (fixed stride: no offset depends on a window), clipped to its stride
  __device__ __forceinline__ uint8_t* plane(int n, int& h, int& w) const {
    const int4 rc = win[n];
    w = rc.z < 1 ? 1 : rc.z;
    h = rc.w < 1 ? 1 : rc.w;
    if ((long long)w > stride) w = (int)stride;
    if ((long long)h * w > stride) h = (int)(stride / w);
    return mask + (size_t)n * stride;
  }
  __device__ __forceinline__ void scales(int h, int w, int H, int W, float& y, float& x) const { plane_scales(h, w, H, W, y, x); }
};

template <typename Planes>
__global__ void extent_init_kernel(int* __restrict__ ext, int N, const Planes planes) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < N) {
    int H, W;
    planes.plane(i, H, W);
    ext[i * 4] = W; ext[i * 4 + 1] = H; ext[i * 4 + 2] = -1; ext[i * 4 + 3] = -1;
  }
}

// One plane pl (f32 [h, w]) -> H x W.  y (the f32 map), mp (u8 {0, 255} of v > thresh) and ext (the extent of the mask, pre-initialised) are each
// optional: the reference's post-processing (circuit_analyzer.py:354-370) only needs the u8 mask and its bounding rectangle, so the f32 map
// need not be written at all.  The value is bil_mix of the four taps: the same roundings whichever kernel inlines this.
__device__ __forceinline__ void bilinear_plane(const float* __restrict__ pl, int h, int w, float sy, float sx, float* __restrict__ y, int H, int W,
                                               uint8_t* __restrict__ mp, float thresh, int* __restrict__ ext) {
  const int total = H * W;
  int ex0 = W, ey0 = H, ex1 = -1, ey1 = -1;
  for (int idx = blockIdx.x * BLOCK + threadIdx.x; idx < total; idx += gridDim.x * BLOCK) {
    const int oy = idx / W, ox = idx - oy * W;
    int y0, y1, x0, x1; float ly, lx;
    bil_axis(oy, sy, h, y0, y1, ly);
    bil_axis(ox, sx, w, x0, x1, lx);
    const float* r0 = pl + (size_t)y0 * w;
    const float* r1 = pl + (size_t)y1 * w;
    const float v = bil_mix(r0[x0], r0[x1], r1[x0], r1[x1], ly, lx);
    if (y) y[idx] = v;
    const bool on = v > thresh;
    if (mp) mp[idx] = on ? 255 : 0;
    if (on) { ex0 = min(ex0, ox); ex1 = max(ex1, ox); ey0 = min(ey0, oy); ey1 = max(ey1, oy); }
  }
  if (ext) extent_fold(ext, ex0, ey0, ex1, ey1);
}

// plane blockIdx.y of x (f32 [N, h, w]) to where `planes` puts it; y (EqualPlanes only) f32 [N, H, W]
template <typename Planes>
__global__ __launch_bounds__(BLOCK) void bilinear_kernel(const float* __restrict__ x, int h, int w, float* __restrict__ y, const Planes planes, float thresh,
                                                      int* __restrict__ ext) {
  const int n = blockIdx.y;
  int H, W;
  float sy, sx;
  uint8_t* mp = planes.plane(n, H, W);
  planes.scales(h, w, H, W, sy, sx);
  bilinear_plane(x + (size_t)n * h * w, h, w, sy, sx, y ? y + (size_t)n * H * W : nullptr, H, W, mp, thresh, ext ? ext + n * 4 : nullptr);
}

// extent[0 .. 4 N) = the empty boxes, then the N planes on a grid of grid_x workgroups each (the entry point sizes it for its largest plane)
template <typename Planes>
inline void launch_mask_return(const float* x, int N, int h, int w, float* y, const Planes& planes, int grid_x, float thresh, int* extent, hipStream_t s) {
  if (extent) hipLaunchKernelGGL(extent_init_kernel<Planes>, dim3((N + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, extent, N, planes);
  hipLaunchKernelGGL(bilinear_kernel<Planes>, dim3(grid_x, N), dim3(BLOCK), 0, s, x, h, w, y, planes, thresh, extent);
}

}  // namespace

extern "C" int cvmi_bilinear_f32(const float* x, int N, int h, int w, float* y, int H, int W, uint8_t* mask_u8, float thresh, cvmi_stream_t stream_) {
  CVMI_CHECK(x && (y || mask_u8) && N > 0 && N <= 65535 && h > 0 && w > 0 && H > 0 && W > 0, "bilinear: bad arguments");
  launch_mask_return(x, N, h, w, y, EqualPlanes(mask_u8, h, w, H, W), grid_for((long long)H * W, 256, 1024), thresh, nullptr, (hipStream_t)stream_);
  CVMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int cvmi_mask_postprocess(const float* x, int N, int h, int w, int H, int W, float thresh, uint8_t* mask_u8, int* extent,
                                     cvmi_stream_t stream_) {
  CVMI_CHECK(x && mask_u8 && extent && N > 0 && N <= 65535 && h > 0 && w > 0 && H > 0 && W > 0, "mask_postprocess: bad arguments");
  launch_mask_return(x, N, h, w, nullptr, EqualPlanes(mask_u8, h, w, H, W), grid_for((long long)H * W, 256, 1024), thresh, extent, (hipStream_t)stream_);
  CVMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int cvmi_mask_postprocess_sizes(const float* x, int N, int h, int w, const int* sizes, float thresh, uint8_t* mask_u8, int* extent,
                                           cvmi_stream_t stream_) {
  CVMI_CHECK(x && mask_u8 && extent && sizes && N > 0 && h > 0 && w > 0, "mask_postprocess_sizes: bad arguments");
  for (int n = 0; n < N; ++n) {                                     // every size before the first launch
    const int H = sizes[2 * (size_t)n], W = sizes[2 * (size_t)n + 1];
    CVMI_CHECK(H > 0 && W > 0 && (long long)H * W < (1ll << 31), "mask_postprocess_sizes: plane %d has size %d x %d", n, H, W);
  }
  for (int n0 = 0; n0 < N; n0 += RECT_MAX) {
    const int nb = N - n0 < RECT_MAX ? N - n0 : RECT_MAX;
    SizedPlanes p;
    p.mask = mask_u8;
    long long maxhw = 1, rel = 0;
    for (int n = 0; n < nb; ++n) {
      const int H = sizes[2 * (size_t)(n0 + n)], W = sizes[2 * (size_t)(n0 + n) + 1];
      p.sz.r[n] = make_int4(H, W, (int)(unsigned)(rel & 0xffffffffll), (int)(unsigned)(rel >> 32));
      rel += (long long)H * W;
      if ((long long)H * W > maxhw) maxhw = (long long)H * W;
    }
    for (int n = nb; n < RECT_MAX; ++n) p.sz.r[n] = make_int4(1, 1, 0, 0);
    launch_mask_return(x + (size_t)n0 * h * w, nb, h, w, nullptr, p, grid_for(maxhw, 256, 1024), thresh, extent + 4 * (size_t)n0, (hipStream_t)stream_);
    CVMI_LAUNCH_CHECK();
    mask_u8 += rel;
  }
  return 0;
}

extern "C" int cvmi_mask_postprocess_rects_dev(const float* x, int N, int h, int w, const int* rects_dev, long long plane_stride, float thresh,
                                               uint8_t* mask_u8, int* extent, cvmi_stream_t stream_) {
  CVMI_CHECK(x && mask_u8 && extent && rects_dev && N > 0 && N <= 65535 && h > 0 && w > 0 && plane_stride > 0 && plane_stride < (1ll << 31) &&
             ((uintptr_t)rects_dev & 15) == 0, "mask_postprocess_rects_dev: bad arguments");
  launch_mask_return(x, N, h, w, nullptr, WindowPlanes{mask_u8, (const int4*)rects_dev, plane_stride}, grid_for(plane_stride, 256, 1024), thresh, extent,
                     (hipStream_t)stream_);
  CVMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int cvmi_mask_extent(const uint8_t* mask, int N, int H, int W, int* extent, cvmi_stream_t stream_) {
  CVMI_CHECK(mask && extent && N > 0 && N <= 65535 && H > 0 && W > 0, "mask_extent: bad arguments");
  hipStream_t s = (hipStream_t)stream_;
  hipLaunchKernelGGL(extent_init_kernel<EqualPlanes>, dim3((N + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, extent, N, EqualPlanes(nullptr, 1, 1, H, W));
  hipLaunchKernelGGL(mask_extent_kernel, dim3(grid_for((long long)H * W, 256, 32), N), dim3(BLOCK), 0, s, mask, H, W, extent);
  CVMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int cvmi_sam2_transform_batch(const uint8_t* src, int B, int H, int W, void* dst, int R, int dst_dtype, int swap_rb, cvmi_stream_t stream_) {
  CVMI_CHECK(src && dst && B >= 1 && B <= 65535 && H > 0 && W > 0 && R > 0, "sam2_transform: bad arguments");
  CVMI_CHECK(is_out_type(dst_dtype), "sam2_transform: bad dtype");
  CVMI_CHECK(taps_fit(H, W, R), "sam2_transform: down-scale factor too large");
  LAUNCH_TRANSFORM(sam2_transform_kernel, dim3(grid_for((long long)R * R), B), (hipStream_t)stream_, dst_dtype, dst, R, swap_rb ? 1 : 0, src, H, W,
                   (float)H / (float)R, (float)W / (float)R);
  return 0;
}

extern "C" int cvmi_sam2_transform(const uint8_t* src, int H, int W, void* dst, int R, int dst_dtype, cvmi_stream_t stream_) {
  return cvmi_sam2_transform_batch(src, 1, H, W, dst, R, dst_dtype, 0, stream_);
}

extern "C" int cvmi_sam2_transform_rects(const uint8_t* src, long long src_image_stride, int H, int W, const int* rects, int B, void* dst, int R,
                                         int dst_dtype, int swap_rb, cvmi_stream_t stream_) {
  CVMI_CHECK(src && dst && rects && B >= 1 && H > 0 && W > 0 && R > 0 && src_image_stride >= 0, "sam2_transform_rects: bad arguments");
  CVMI_CHECK(is_out_type(dst_dtype), "sam2_transform_rects: bad dtype");
  for (int b = 0; b < B; ++b) {                                     // every window before the first launch: a bad one leaves nothing half done
    const int* r = rects + 4 * (size_t)b;
    CVMI_CHECK(window_inside(r[0], r[1], r[2], r[3], W, H), "sam2_transform_rects: window %d = (x %d, y %d, w %d, h %d) leaves the %d x %d image", b,
               r[0], r[1], r[2], r[3], W, H);
    CVMI_CHECK(taps_fit(r[3], r[2], R), "sam2_transform_rects: down-scale factor of window %d too large", b);
  }
  for (int b0 = 0; b0 < B; b0 += RECT_MAX) {
    const int nb = B - b0 < RECT_MAX ? B - b0 : RECT_MAX;
    RectTable t;
    for (int b = 0; b < RECT_MAX; ++b) {
      const int* r = rects + 4 * (size_t)(b0 + (b < nb ? b : 0));
      t.r[b] = make_int4(r[0], r[1], r[2], r[3]);
    }
    LAUNCH_TRANSFORM(sam2_transform_rects_kernel, dim3(grid_for((long long)R * R), nb), (hipStream_t)stream_, dst_dtype,
                     (char*)dst + (size_t)b0 * R * R * 3 * out_bytes(dst_dtype), R, swap_rb ? 1 : 0, src + (size_t)b0 * src_image_stride, src_image_stride, W, t);
  }
  return 0;
}

extern "C" int cvmi_sam2_transform_rects_dev(const uint8_t* src, long long src_image_stride, int H, int W, const int* rects_dev, int B, void* dst, int R,
                                             int dst_dtype, int swap_rb, cvmi_stream_t stream_) {
  CVMI_CHECK(src && dst && rects_dev && B >= 1 && B <= 65535 && H > 0 && W > 0 && R > 0 && src_image_stride >= 0 && ((uintptr_t)rects_dev & 15) == 0,
             "sam2_transform_rects_dev: bad arguments");
  CVMI_CHECK(is_out_type(dst_dtype), "sam2_transform_rects_dev: bad dtype");
  CVMI_CHECK(taps_fit(H, W, R), "sam2_transform_rects_dev: down-scale factor of the %d x %d image too large", W, H);   // the whole image bounds every window inside it
  LAUNCH_TRANSFORM(sam2_transform_rects_dev_kernel, dim3(grid_for((long long)R * R), B), (hipStream_t)stream_, dst_dtype, dst, R, swap_rb ? 1 : 0, src,
                   src_image_stride, H, W, (const int4*)rects_dev);
  return 0;
}

extern "C" int cvmi_sam2_transform_srcs(const uint8_t* src, long long src_bytes, const cvmi_sam2_src_row* rows, int B, void* dst, int R, int dst_dtype,
                                        int swap_rb, cvmi_stream_t stream_) {
  CVMI_CHECK(src && dst && rows && B >= 1 && R > 0 && src_bytes > 0, "sam2_transform_srcs: bad arguments");
  CVMI_CHECK(is_out_type(dst_dtype), "sam2_transform_srcs: bad dtype");
  for (int b = 0; b < B; ++b) {                                     // every row before the first launch
    const cvmi_sam2_src_row& r = rows[b];
    CVMI_CHECK(r.H > 0 && r.W > 0 && r.src_byte_offset >= 0 && r.src_byte_offset + (long long)r.H * r.W * 3 <= src_bytes,
               "sam2_transform_srcs: row %d: %d x %d x 3 bytes at offset %lld leave the %lld-byte source buffer", b, r.H, r.W, r.src_byte_offset, src_bytes);
    CVMI_CHECK(window_inside(r.x0, r.y0, r.w, r.h, r.W, r.H), "sam2_transform_srcs: window %d = (x %d, y %d, w %d, h %d) leaves the %d x %d image", b,
               r.x0, r.y0, r.w, r.h, r.W, r.H);
    CVMI_CHECK(taps_fit(r.h, r.w, R), "sam2_transform_srcs: down-scale factor of window %d too large", b);
  }
  for (int b0 = 0; b0 < B; b0 += RECT_MAX) {
    const int nb = B - b0 < RECT_MAX ? B - b0 : RECT_MAX;
    SrcTable t;
    for (int b = 0; b < RECT_MAX; ++b) t.r[b] = rows[b0 + (b < nb ? b : 0)];
    LAUNCH_TRANSFORM(sam2_transform_srcs_kernel, dim3(grid_for((long long)R * R), nb), (hipStream_t)stream_, dst_dtype,
                     (char*)dst + (size_t)b0 * R * R * 3 * out_bytes(dst_dtype), R, swap_rb ? 1 : 0, src, t);
  }
  return 0;
}
