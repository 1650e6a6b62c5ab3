// The glue between the detector and the segmenter, on the device: scale_boxes -> round -> stage-2 NMS -> crop window -> box shift
// (detector.py scale_boxes / non_max_suppression_by_confidence, pipeline.py results_to_bboxes, crop.py crop_window / adjust_bboxes; the
// reference's analysis_pipeline.py:97-115 and circuit_analyzer.py:937-1284).  One workgroup of 256 threads per image, all state in LDS:
// a latency kernel -- what it buys is that the segmenter's transform can read its window from HBM without the host in between.
// Built with -ffp-contract=off (Makefile): every f64 expression below is the host code's expression, one rounding per operation.
#include "common.hpp"

#include <limits.h>

#ifndef CVMI_OPERAND_BF16          // type-independent: one copy, whichever operand type this translation unit is built for

namespace {

constexpr int GL_CAP = CVMI_GLUE_MAX_DET;            // boxes per image the LDS tables hold
constexpr int GL_WORDS = (GL_CAP + 31) / 32;         // adjacency row: one bit per element
constexpr int GL_SLOTS = (GL_CAP + 255) / 256;       // elements a thread owns
constexpr int GL_HEAD = CVMI_GLUE_INFO_HEAD;
enum { GF_NOT_CLUSTERED = CVMI_GLUE_CLASS_NOT_CLUSTERED, GF_JUNCTION = CVMI_GLUE_CLASS_JUNCTION, GF_TEXT = CVMI_GLUE_CLASS_TEXT,
       GF_NON_COMPONENT = CVMI_GLUE_CLASS_NON_COMPONENT };                           // the class-flag table's bits (glue.py class_flags)
constexpr double TEXT_PADDING = 20.0, TEXT_REACH = 150.0;                            // circuit_analyzer.py:1192, :1201

struct GlueArgs {
  const float* det; const int* count; int max_det, H0, W0; float gain; int pad_x, pad_y; double iou; int padding;
  const uint8_t* flags; int n_flags;
  int *kept_idx, *kept_count, *boxes, *adj_boxes, *window, *info;
};

// crop.py _near on one pair: the boxes overlap (closed intervals) or both axis gaps are <= dist
__device__ __forceinline__ bool near_boxes(const int* a, const int* b, double dist) {
  const double gx = fmax(fmax((double)b[0] - (double)a[2], (double)a[0] - (double)b[2]), 0.0);
  const double gy = fmax(fmax((double)b[1] - (double)a[3], (double)a[1] - (double)b[3]), 0.0);
  return gx <= dist && gy <= dist;
}

__device__ __forceinline__ void put_f64(int* p, double v) {
  const long long b = __double_as_longlong(v);
  p[0] = (int)(unsigned)(b & 0xffffffffll);
  p[1] = (int)(unsigned)((unsigned long long)b >> 32);
}

__global__ __launch_bounds__(256) void stage2_crop_kernel(const GlueArgs a) {
  __shared__ int s_box[GL_CAP][4];                   // rounded boxes in original pixels, detector order
  __shared__ float s_conf[GL_CAP];
  __shared__ uint8_t s_fl[GL_CAP];                   // class flags, detector order
  __shared__ int s_ord[GL_CAP];                      // confidence rank -> detector index
  __shared__ uint8_t s_alive[GL_CAP];                // by confidence rank
  __shared__ int s_kept[GL_CAP];                     // kept position -> detector index
  __shared__ uint8_t s_bflag[GL_CAP];                // by kept position: bit 0 = this text box expanded the window
  __shared__ int s_e[GL_CAP], s_t[GL_CAP];           // element / text position -> kept position (both ascending)
  __shared__ unsigned s_adj[GL_CAP][GL_WORDS];
  __shared__ int s_label[GL_CAP], s_size[GL_CAP], s_wt[GL_CAP], s_nc[GL_CAP];
  __shared__ int s_i[16];                            // scalars lane 0 decides, see the names below
  __shared__ double s_d[2];
  __shared__ int s_changed;
  enum { I_NE, I_NT, I_LINK, I_ROOT, I_BX0, I_BY0, I_BX1, I_BY1, I_APPLIED, I_WX0, I_WY0, I_WX1, I_WY1, I_STOP };

  const int img = blockIdx.x, tid = threadIdx.x, md = a.max_det;
  int n = a.count[img];
  n = n < 0 ? 0 : n > md ? md : n;
  const float* det = a.det + (size_t)img * md * 6;
  int* o_kept = a.kept_idx + (size_t)img * md;
  int* o_box = a.boxes + (size_t)img * md * 4;
  int* o_adj = a.adj_boxes + (size_t)img * md * 4;
  int* o_info = a.info + (size_t)img * (GL_HEAD + md);
  const int H0 = a.H0, W0 = a.W0;

  // (a) scale_boxes in f32: minus the pad, DIVIDED by the gain, clamped; (b) np.rint of the f64 copy
  for (int i = tid; i < n; i += 256) {
    const float* d = det + (size_t)i * 6;
    const float px = (float)a.pad_x, py = (float)a.pad_y, w = (float)W0, h = (float)H0;
    const float x1 = fminf(fmaxf((d[0] - px) / a.gain, 0.f), w), y1 = fminf(fmaxf((d[1] - py) / a.gain, 0.f), h);
    const float x2 = fminf(fmaxf((d[2] - px) / a.gain, 0.f), w), y2 = fminf(fmaxf((d[3] - py) / a.gain, 0.f), h);
    const int b[4] = {(int)rint((double)x1), (int)rint((double)y1), (int)rint((double)x2), (int)rint((double)y2)};
#pragma unroll
    for (int c = 0; c < 4; ++c) { s_box[i][c] = b[c]; o_box[i * 4 + c] = b[c]; }
    s_conf[i] = d[4];
    const int cls = (int)d[5];
    s_fl[i] = cls >= 0 && cls < a.n_flags ? a.flags[cls] : 0;
    s_alive[i] = 1;
    s_bflag[i] = 0;
  }
  if (tid < 16) s_i[tid] = 0;
  __syncthreads();

  // (c) stable descending rank by confidence: a counting rank per box
  const bool nms = a.iou >= 0.0;
  for (int i = tid; i < n; i += 256) {
    int r = i;
    if (nms) {
      const float c = s_conf[i];
      r = 0;
      for (int j = 0; j < n; ++j) r += (s_conf[j] > c) || (s_conf[j] == c && j < i);
    }
    s_ord[r] = i;
  }
  __syncthreads();

  // (d) utils.py:346-361: the kept candidates in turn, the rest of the list in parallel; calculate_iou's operations in f64
  int K = 0;
  if (nms) {
    for (int i = 0; i < n; ++i) {
      __syncthreads();
      if (!s_alive[i]) continue;                     // (uniform: written before the barrier)
      const int* bi = s_box[s_ord[i]];
      if (tid == 0) s_kept[K] = s_ord[i];
      ++K;
      const double ix0 = bi[0], iy0 = bi[1], ix1 = bi[2], iy1 = bi[3];
      const double area_i = (ix1 - ix0) * (iy1 - iy0);
      for (int r = i + 1 + tid; r < n; r += 256) {
        if (!s_alive[r]) continue;
        const int* br = s_box[s_ord[r]];
        const double rx0 = br[0], ry0 = br[1], rx1 = br[2], ry1 = br[3];
        const double iw = fmax(fmin(ix1, rx1) - fmax(ix0, rx0), 0.0), ih = fmax(fmin(iy1, ry1) - fmax(iy0, ry0), 0.0);
        const double inter = iw * ih;
        const double uni = (area_i + (rx1 - rx0) * (ry1 - ry0)) - inter;
        const double iou = uni > 0.0 ? inter / uni : 0.0;
        if (!(iou < a.iou)) s_alive[r] = 0;
      }
    }
  } else {
    for (int i = tid; i < n; i += 256) s_kept[i] = i;
    K = n;
  }
  __syncthreads();
  for (int k = tid; k < K; k += 256) o_kept[k] = s_kept[k];

  // (e) crop.py crop_window on the kept list.  Lane 0 walks the list once, in list order: the element and text sets, the class counts and
  //     the width / height sums exactly as the host adds them up.
  if (tid == 0) {
    int ne = 0, nt = 0, ncomp_type = 0, ncomp = 0;
    for (int k = 0; k < K; ++k) {
      const int f = s_fl[s_kept[k]];
      ncomp_type += !(f & GF_NON_COMPONENT);
      if (f & GF_TEXT) s_t[nt++] = k;
      if (!(f & GF_NOT_CLUSTERED)) { s_e[ne++] = k; ncomp += !(f & GF_JUNCTION); }
    }
    s_i[I_NE] = ne; s_i[I_NT] = nt;
    for (int w = 0; w < GL_HEAD; ++w) o_info[w] = 0;
    o_info[CVMI_GLUE_LINK] = o_info[CVMI_GLUE_CLUSTERS] = o_info[CVMI_GLUE_MAIN_FIRST] = -1;
    o_info[CVMI_GLUE_TOTAL] = K; o_info[CVMI_GLUE_COMPONENT_TYPE] = ncomp_type; o_info[CVMI_GLUE_TEXT_TYPE] = nt; o_info[CVMI_GLUE_PADDING] = a.padding;
    if (ne == 0) {
      o_info[CVMI_GLUE_REASON] = CVMI_GLUE_REASON_NO_ELEMENTS; o_info[CVMI_GLUE_DECISION] = CVMI_GLUE_DECISION_NO_ELEMENTS;
      s_i[I_STOP] = 1;
    } else {
      const bool any_comp = ncomp > 0;               // components set the scale; junctions only when there is nothing else (:1003-1017)
      double sw = 0.0, sh = 0.0;
      int cnt = 0;
      for (int e = 0; e < ne; ++e) {
        const int* b = s_box[s_kept[s_e[e]]];
        if (any_comp && (s_fl[s_kept[s_e[e]]] & GF_JUNCTION)) continue;
        sw += (double)b[2] - (double)b[0]; sh += (double)b[3] - (double)b[1]; ++cnt;
      }
      const double mw = sw / (double)cnt, mh = sh / (double)cnt;
      const double diag = sqrt(mw * mw + mh * mh);
      const int link0 = (int)(diag * (any_comp ? 2.0 : 2.5)), floor0 = any_comp ? 30 : 20;
      const int link = link0 > floor0 ? link0 : floor0;
      const int td0 = (int)((diag > 0.0 ? diag : 30.0) * 0.75);
      s_i[I_LINK] = link;
      s_d[0] = (double)link; s_d[1] = (double)(td0 > 25 ? td0 : 25);
      o_info[CVMI_GLUE_LINK] = link;
    }
  }
  __syncthreads();
  const int ne = s_i[I_NE], nt = s_i[I_NT];
  if (!s_i[I_STOP]) {
    const double link = s_d[0], text_dist = s_d[1];
    // pairwise _near adjacency (bit j of row e), labels = own index
    for (int it = tid; it < ne * GL_WORDS; it += 256) {
      const int e = it / GL_WORDS, w = it - e * GL_WORDS;
      const int* be = s_box[s_kept[s_e[e]]];
      unsigned bits = 0;
      for (int j = w * 32; j < w * 32 + 32 && j < ne; ++j) bits |= (unsigned)near_boxes(be, s_box[s_kept[s_e[j]]], link) << (j & 31);
      s_adj[e][w] = bits;
    }
    for (int e = tid; e < ne; e += 256) { s_label[e] = e; s_size[e] = s_wt[e] = s_nc[e] = 0; }
    // connected components: label = lowest member index, by min-propagation (+ pointer jumping) to the fixed point
    do {
      __syncthreads();
      if (tid == 0) s_changed = 0;
      int m[GL_SLOTS];
#pragma unroll
      for (int q = 0; q < GL_SLOTS; ++q) {
        const int e = tid + 256 * q;
        m[q] = GL_CAP;
        if (e < ne) {
          m[q] = s_label[e];
          for (int w = 0; w < GL_WORDS; ++w) {
            unsigned bits = s_adj[e][w];
            while (bits) { const int j = w * 32 + __builtin_ctz(bits); bits &= bits - 1; m[q] = min(m[q], s_label[j]); }
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < GL_SLOTS; ++q) {
        const int e = tid + 256 * q;
        if (e < ne && m[q] < s_label[e]) { s_label[e] = m[q]; s_changed = 1; }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < GL_SLOTS; ++q) { const int e = tid + 256 * q; if (e < ne) m[q] = s_label[s_label[e]]; }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < GL_SLOTS; ++q) { const int e = tid + 256 * q; if (e < ne) s_label[e] = m[q]; }
      __syncthreads();
    } while (s_changed);
    // per cluster (at its root): size, components with a text box within text_dist, components
    for (int e = tid; e < ne; e += 256) {
      const int k = s_kept[s_e[e]], root = s_label[e];
      const bool comp = !(s_fl[k] & GF_JUNCTION);
      bool has_text = false;
      if (comp)
        for (int t = 0; t < nt && !has_text; ++t) has_text = near_boxes(s_box[k], s_box[s_kept[s_t[t]]], text_dist);
      atomicAdd(&s_size[root], 1);
      if (has_text) atomicAdd(&s_wt[root], 1);
      if (comp) atomicAdd(&s_nc[root], 1);
    }
    __syncthreads();
    // the two-step pick: the first lexicographic maximum of (text associations, size); without any association in a cluster that has
    // components, the first of the largest clusters
    if (tid == 0) {
      int nclu = 0, best = -1, best_id = 0, big = -1, big_id = 0;
      for (int e = 0; e < ne; ++e) {
        if (s_label[e] != e) continue;
        if (best < 0 || s_wt[e] > s_wt[best] || (s_wt[e] == s_wt[best] && s_size[e] > s_size[best])) { best = e; best_id = nclu; }
        if (big < 0 || s_size[e] > s_size[big]) { big = e; big_id = nclu; }
        ++nclu;
      }
      const bool fallback = s_wt[best] == 0 && s_nc[best] > 0;
      const int pick = fallback ? big : best;
      o_info[CVMI_GLUE_CLUSTERS] = nclu;
      o_info[CVMI_GLUE_DECISION] = fallback ? CVMI_GLUE_DECISION_FALLBACK : CVMI_GLUE_DECISION_SCORED;
      o_info[CVMI_GLUE_MAIN_SIZE] = s_size[pick]; o_info[CVMI_GLUE_MAIN_TEXT] = s_wt[pick];
      o_info[CVMI_GLUE_MAIN_ID] = fallback ? big_id : best_id;
      o_info[CVMI_GLUE_MAIN_FIRST] = s_e[pick];      // the root IS the cluster's lowest member
      s_i[I_ROOT] = pick;
      s_i[I_BX0] = s_i[I_BY0] = INT_MAX; s_i[I_BX1] = s_i[I_BY1] = INT_MIN;
    }
    __syncthreads();
    for (int e = tid; e < ne; e += 256) {
      if (s_label[e] != s_i[I_ROOT]) continue;
      const int* b = s_box[s_kept[s_e[e]]];
      atomicMin(&s_i[I_BX0], b[0]); atomicMin(&s_i[I_BY0], b[1]); atomicMax(&s_i[I_BX1], b[2]); atomicMax(&s_i[I_BY1], b[3]);
    }
    __syncthreads();
    // basis box, the > 0.90 area test, padding + clamp, the text growth (sequential: each text box sees the window the previous ones
    // left), rounding, validity
    if (tid == 0) {
      const double bx0 = s_i[I_BX0], by0 = s_i[I_BY0], bx1 = s_i[I_BX1], by1 = s_i[I_BY1], W = (double)W0, H = (double)H0;
      put_f64(o_info + CVMI_GLUE_BASIS, bx0); put_f64(o_info + CVMI_GLUE_BASIS + 2, by0);
      put_f64(o_info + CVMI_GLUE_BASIS + 4, bx1); put_f64(o_info + CVMI_GLUE_BASIS + 6, by1);
      o_info[CVMI_GLUE_BASIS_SET] = 1;
      const double area = (double)((long long)H0 * W0);
      if (area > 0.0 && (fmax(0.0, bx1 - bx0) * fmax(0.0, by1 - by0)) / area > 0.90) {
        o_info[CVMI_GLUE_REASON] = CVMI_GLUE_REASON_TOO_LARGE;
      } else {
        const double pad = (double)a.padding;
        double x0 = fmax(0.0, bx0 - pad), y0 = fmax(0.0, by0 - pad), x1 = fmin(W, bx1 + pad), y1 = fmin(H, by1 + pad);
        o_info[CVMI_GLUE_PADDED] = (int)rint(x0); o_info[CVMI_GLUE_PADDED + 1] = (int)rint(y0);
        o_info[CVMI_GLUE_PADDED + 2] = (int)rint(x1); o_info[CVMI_GLUE_PADDED + 3] = (int)rint(y1);
        o_info[CVMI_GLUE_PADDED_SET] = 1;
        for (int t = 0; t < nt; ++t) {
          const int* b = s_box[s_kept[s_t[t]]];
          const double tx0 = b[0], ty0 = b[1], tx1 = b[2], ty1 = b[3];
          if (tx1 < x0 - TEXT_REACH || tx0 > x1 + TEXT_REACH || ty1 < y0 - TEXT_REACH || ty0 > y1 + TEXT_REACH) continue;
          const double nx0 = fmin(x0, fmax(0.0, tx0 - TEXT_PADDING)), ny0 = fmin(y0, fmax(0.0, ty0 - TEXT_PADDING));
          const double nx1 = fmax(x1, fmin(W, tx1 + TEXT_PADDING)), ny1 = fmax(y1, fmin(H, ty1 + TEXT_PADDING));
          if (nx0 != x0 || ny0 != y0 || nx1 != x1 || ny1 != y1) s_bflag[s_t[t]] = 1;
          x0 = nx0; y0 = ny0; x1 = nx1; y1 = ny1;
        }
        const int wx0 = max(0, (int)rint(x0)), wy0 = max(0, (int)rint(y0)), wx1 = min(W0, (int)rint(x1)), wy1 = min(H0, (int)rint(y1));
        o_info[CVMI_GLUE_FINAL] = wx0; o_info[CVMI_GLUE_FINAL + 1] = wy0; o_info[CVMI_GLUE_FINAL + 2] = wx1; o_info[CVMI_GLUE_FINAL + 3] = wy1;
        o_info[CVMI_GLUE_FINAL_SET] = 1;
        if (wx0 >= wx1 || wy0 >= wy1) {
          o_info[CVMI_GLUE_REASON] = CVMI_GLUE_REASON_INVALID;
        } else {
          o_info[CVMI_GLUE_APPLIED] = 1;
          s_i[I_APPLIED] = 1; s_i[I_WX0] = wx0; s_i[I_WY0] = wy0; s_i[I_WX1] = wx1; s_i[I_WY1] = wy1;
        }
      }
    }
  }
  __syncthreads();

  // (f) adjust_bboxes: every kept box in the window's coordinates, clipped to it; the window itself as {x0, y0, w, h}
  const bool applied = s_i[I_APPLIED] != 0;
  const int wx0 = applied ? s_i[I_WX0] : 0, wy0 = applied ? s_i[I_WY0] : 0;
  const int ww = applied ? s_i[I_WX1] - wx0 : W0, wh = applied ? s_i[I_WY1] - wy0 : H0;
  for (int k = tid; k < K; k += 256) {
    const int* b = s_box[s_kept[k]];
    int q[4] = {b[0], b[1], b[2], b[3]}, dropped = 0;
    if (applied) {
      q[0] = max(0, b[0] - wx0); q[1] = max(0, b[1] - wy0); q[2] = min(ww, b[2] - wx0); q[3] = min(wh, b[3] - wy0);
      dropped = !(q[2] > q[0] && q[3] > q[1]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) o_adj[k * 4 + c] = q[c];
    o_info[GL_HEAD + k] = (s_bflag[k] ? CVMI_GLUE_BOX_EXPANDED : 0) | (dropped ? CVMI_GLUE_BOX_DROPPED : 0);
  }
  if (tid == 0) {
    a.kept_count[img] = K;
    int* w = a.window + (size_t)img * 4;
    w[0] = wx0; w[1] = wy0; w[2] = ww; w[3] = wh;
  }
}

}  // namespace

extern "C" int cvmi_stage2_crop(const float* det, const int* count, int B, int max_det, int H0, int W0, float gain, int pad_x, int pad_y,
                                double stage2_iou, int padding, const uint8_t* class_flags, int n_flags, int* kept_idx, int* kept_count,
                                int* boxes, int* adj_boxes, int* window, int* info, cvmi_stream_t stream_) {
  CVMI_CHECK(max_det >= 1 && max_det <= GL_CAP, "stage2_crop: max_det = %d, this build holds at most %d boxes per image", max_det, GL_CAP);
  CVMI_CHECK(det && count && class_flags && kept_idx && kept_count && boxes && adj_boxes && window && info, "stage2_crop: null pointer");
  CVMI_CHECK(B >= 1 && H0 >= 1 && W0 >= 1 && (long long)H0 * W0 < (1ll << 31) && gain > 0.f && n_flags >= 0 && padding >= 0 && stage2_iou == stage2_iou,
             "stage2_crop: bad arguments");
  const GlueArgs a = {det, count, max_det, H0, W0, gain, pad_x, pad_y, stage2_iou, padding, class_flags, n_flags,
                      kept_idx, kept_count, boxes, adj_boxes, window, info};
  cvmi_note_kernel("stage2_crop_kernel");
  hipLaunchKernelGGL(stage2_crop_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream_, a);
  CVMI_LAUNCH_CHECK();
  return 0;
}

#endif  // CVMI_OPERAND_BF16
