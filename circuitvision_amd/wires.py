"""Node-analysis front end on the device: the step that consumes the segmenter's mask.

What it restates is the start of CircuitAnalyzer.get_node_connections (/root/reference/src/circuit_analyzer.py:1286-1370), which the
reference runs per image on the host through OpenCV (run_node_analysis, src/analysis_pipeline.py:227):

    empty the component boxes           :1327-1345   cvmi_node_prepare     (wire_ops.hip)
    resize_image_keep_aspect(600)       :787-809     cvmi_node_prepare     (cv2.resize INTER_LINEAR) + resize_bboxes :461-477 on the host
    enhance_lines                       :289-311     cvmi_enhance_lines    (blur -> dilate -> erode, fused, + exact plane sums)
    get_contours                        :388-459     cvmi_external_contours (labelling + border tracing) + the area filter on the host

A batch stays in HBM until it comes back as contour points.  `contour_img`, the drawing get_contours returns second (drawContours +
putText), is NOT rendered: a zero uint8 [H, W, 3] canvas stands in for it, so that callers that take `.copy()` of it run unchanged.
"""
import numpy as np
import torch

from . import _lib

PRESERVED = ("crossover", "junction", "circuit", "vss")       # circuit_analyzer.py:1332: classes whose boxes stay in the mask


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _to_device_u8(img):
    """-> (contiguous u8 [H, W] device tensor, was numpy)."""
    if isinstance(img, np.ndarray):
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError(f"expected a uint8 [H, W] plane, got {img.dtype} {img.shape}")
        return torch.from_numpy(np.ascontiguousarray(img)).to(_dev()), True
    if not torch.is_tensor(img) or img.dtype != torch.uint8 or img.dim() != 2 or not img.is_cuda:
        raise ValueError("expected a uint8 [H, W] numpy plane or device tensor")
    return img.contiguous(), False


def _sizes(shapes, cols=2):
    return np.ascontiguousarray(np.asarray(shapes, dtype=np.int32).reshape(-1, cols))


def _pack(planes):
    """-> (one packed u8 device buffer, per-plane offsets)."""
    offs = np.concatenate(([0], np.cumsum([p.numel() for p in planes], dtype=np.int64)))
    if len(planes) == 1:
        return planes[0].contiguous().view(-1), offs
    return torch.cat([p.reshape(-1) for p in planes]), offs


def _views(buf, offs, shapes):
    return [buf[int(offs[i]):int(offs[i + 1])].view(h, w) for i, (h, w) in enumerate(shapes)]


# ---- the three device stages on packed planes ------------------------------------------------------------------------------------
def new_width(H, W, new_height=600):
    """resize_image_keep_aspect :799-803, in python float64."""
    nw = int(new_height * (W / H))
    if nw <= 0:
        raise ValueError(f"a {H} x {W} mask resized to height {new_height} has no width (cv2.resize would reject it)")
    return nw


def prepare_packed(src, shapes, bboxes, new_height=600):
    """Empty the boxes and resize to `new_height` for packed planes: -> (emptied buf, resized buf, resized shapes)."""
    lib = _lib.load()
    new_shapes = [(new_height, new_width(h, w, new_height)) for h, w in shapes]
    rows, start = [], [0]
    for (h, w), bb in zip(shapes, bboxes):
        for b in bb:
            if b["class"] not in PRESERVED:                          # int() truncates as the reference's int(bbox[...]) does
                rows.append([min(max(int(b[k]), -1), lim + 1) for k, lim in (("xmin", w), ("ymin", h), ("xmax", w), ("ymax", h))])
        start.append(len(rows))
    boxes = torch.tensor(rows, dtype=torch.int32).reshape(-1, 4).to(src.device) if rows else None
    start = np.asarray(start, dtype=np.int32)
    sizes = _sizes([(h, w, nh, nw) for (h, w), (nh, nw) in zip(shapes, new_shapes)], 4)
    emptied = torch.empty_like(src)
    resized = torch.empty(sum(h * w for h, w in new_shapes), dtype=torch.uint8, device=src.device)
    _lib.check(lib.cvmi_node_prepare(src.data_ptr(), len(shapes), sizes.ctypes.data, boxes.data_ptr() if boxes is not None else None,
                                     start.ctypes.data, emptied.data_ptr(), resized.data_ptr(), _stream()), "node_prepare")
    return emptied, resized, new_shapes


def enhance_packed(src, shapes):
    """enhance_lines on packed planes: -> (enhanced buf, exact u64 plane sums as int64 [N])."""
    lib = _lib.load()
    sizes = _sizes(shapes)
    dst = torch.empty_like(src)
    sums = torch.empty(len(shapes), dtype=torch.int64, device=src.device)
    _lib.check(lib.cvmi_enhance_lines(src.data_ptr(), len(shapes), sizes.ctypes.data, dst.data_ptr(), sums.data_ptr(), _stream()), "enhance_lines")
    return dst, sums


class PackedContours:
    """External contours of N packed planes, on the host: per contour its plane, points (int32 [n, 2]), 2 x signed area, rectangle."""

    def __init__(self, counts, info, area2, points):
        self.counts, self.info, self.area2, self.points = counts, info, area2, points
        self.longest_border = int(counts[-1])

    def plane(self, n):
        lo = int(self.counts[:n].sum())
        hi = lo + int(self.counts[n])
        out = []
        for c in range(lo, hi):
            _, npts, off, x, y, w, h, _steps = self.info[c].tolist()
            out.append((self.points[off:off + npts], int(self.area2[c]), (x, y, w, h)))
        return out


def contours_packed(planes, shapes, sums=None, binarize=True, cap_contours=None, cap_points=None):
    """findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) of packed planes (`sums`: the planes' exact sums, int64 device [N], for
    get_contours' inversion; None = no inversion).  binarize: planes that do not invert get the reference's img[img == 255] = 1 in place.
    The first-guess capacities are raised to the true totals and the call repeated when they are short: nothing is truncated."""
    lib = _lib.load()
    N = len(shapes)
    sizes = _sizes(shapes)
    dev = planes.device
    ws_bytes = int(lib.cvmi_contours_workspace(N, sizes.ctypes.data))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(N + 3, dtype=torch.int32, device=dev)
    cc = int(cap_contours) if cap_contours is not None else 512 * N
    cp = int(cap_points) if cap_points is not None else 32768 * N
    for _ in range(2):
        info = torch.empty(max(cc, 1), 8, dtype=torch.int32, device=dev)
        area2 = torch.empty(max(cc, 1), dtype=torch.int64, device=dev)
        points = torch.empty(max(cp, 1), 2, dtype=torch.int32, device=dev)
        _lib.check(lib.cvmi_external_contours(planes.data_ptr(), sums.data_ptr() if sums is not None else None, N, sizes.ctypes.data,
                                              int(bool(binarize)), ws.data_ptr(), ws_bytes, cc, cp, counts.data_ptr(), info.data_ptr(),
                                              area2.data_ptr(), points.data_ptr(), _stream()), "external_contours")
        c = counts.cpu().numpy()
        nc, npt = int(c[N]), int(c[N + 1])
        if nc <= cc and npt <= cp:
            return PackedContours(np.concatenate((c[:N], c[N + 2:])), info[:nc].cpu().numpy(), area2[:nc].cpu().numpy(),
                                  points[:npt].cpu().numpy())
        cc, cp = max(cc, nc), max(cp, npt)
    raise _lib.CvmiError("external_contours: totals changed between two calls on the same planes")


def contour_dicts(plane_contours, H, W, area_threshold=0.0004):
    """get_contours :408-411: contourArea(c) / (H * W) > area_threshold, ids after filtering, boundingRect."""
    norm = H * W
    out = []
    for pts, a2, rect in plane_contours:
        area = abs(a2) / 2.0                                          # contourArea: |shoelace| / 2, exact in double for integer points
        if area / norm > area_threshold:
            out.append({"id": len(out), "contour": np.ascontiguousarray(pts, dtype=np.int32).reshape(-1, 1, 2), "area": area / norm,
                        "rectangle": tuple(int(v) for v in rect)})
    return out


# ---- the reference's two methods ----------------------------------------------------------------------------------------------
def enhance_lines(image):
    """CircuitAnalyzer.enhance_lines (circuit_analyzer.py:289-311) on a u8 [H, W] numpy plane (-> numpy) or device tensor (-> tensor)."""
    x, was_np = _to_device_u8(image)
    y, _ = enhance_packed(x.view(-1), [tuple(x.shape)])
    y = y.view(x.shape)
    return y.cpu().numpy() if was_np else y


def get_contours(img, area_threshold=0.00040):
    """CircuitAnalyzer.get_contours (circuit_analyzer.py:388-459): -> (contour dicts, contour_img).  contour_img is a zero uint8 [H, W, 3]
    canvas: the drawing is not rendered.  A numpy plane that does not invert is changed in place (img[img == 255] = 1) as in the
    reference; a device tensor likewise."""
    x, was_np = _to_device_u8(img)
    H, W = x.shape
    flat = x.view(-1)
    sums = flat.sum(dtype=torch.int64).reshape(1)                    # the enhance stage produces these in the batched path
    pc = contours_packed(flat, [(H, W)], sums, binarize=True)
    if was_np:
        if int(sums.item()) <= 127 * H * W:
            img[img == 255] = 1
    elif x.data_ptr() != img.data_ptr():
        img.copy_(x)
    return contour_dicts(pc.plane(0), H, W, area_threshold), np.zeros((H, W, 3), dtype=np.uint8)


def node_contours(masks, bboxes, new_height=600, area_threshold=0.0004, events=None):
    """get_node_connections up to get_contours (circuit_analyzer.py:1325-1365) for a batch of u8 device masks [H_i, W_i] and their
    crop-relative boxes, in three launches over all planes.  -> per image {"emptied_mask": u8 [H, W] device (before the resize),
    "resized_bboxes": resize_bboxes' dicts, "enhanced": u8 [new_height, new_w] device as the reference leaves `enhanced` after
    get_contours (255 -> 1 where the plane did not invert), "contours": get_contours' dicts}.
    events: optional list that receives (name, torch.cuda.Event) pairs around the sub-stages (tools/node_stage_bench.py)."""
    if not masks:
        return []
    planes = [m if m.is_contiguous() else m.contiguous() for m in masks]
    shapes = [tuple(m.shape) for m in planes]

    def mark(name):
        if events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events.append((name, e))
    mark("start")
    src, offs = _pack(planes)
    mark("pack")
    emptied, resized, new_shapes = prepare_packed(src, shapes, bboxes, new_height)
    mark("prepare")
    enhanced, sums = enhance_packed(resized, new_shapes)
    mark("enhance")
    pc = contours_packed(enhanced, new_shapes, sums, binarize=True)
    mark("contours")
    roffs = np.concatenate(([0], np.cumsum([h * w for h, w in new_shapes], dtype=np.int64)))
    em, en = _views(emptied, offs, shapes), _views(enhanced, roffs, new_shapes)
    out = []
    for i, ((h, w), (nh, nw)) in enumerate(zip(shapes, new_shapes)):
        sx, sy = nw / w, nh / h
        rb = []
        for b in bboxes[i]:
            r = dict(b)
            r["xmin"], r["ymin"], r["xmax"], r["ymax"] = int(b["xmin"] * sx), int(b["ymin"] * sy), int(b["xmax"] * sx), int(b["ymax"] * sy)
            rb.append(r)
        out.append({"emptied_mask": em[i], "resized_bboxes": rb, "enhanced": en[i],
                    "contours": contour_dicts(pc.plane(i), nh, nw, area_threshold)})
    if events is not None:
        events.append(("longest_border", pc.longest_border))
    return out
