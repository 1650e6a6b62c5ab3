"""Node-analysis front end on the device: the step that consumes the segmenter's mask.

What it restates is the start of CircuitAnalyzer.get_node_connections (/root/reference/src/circuit_analyzer.py:1286-1370), which the
reference runs per image on the host through OpenCV (run_node_analysis, src/analysis_pipeline.py:227):

    empty the component boxes           :1327-1345   cvmi_node_prepare     (wire_ops.hip)
    resize_image_keep_aspect(600)       :787-809     cvmi_node_prepare     (cv2.resize INTER_LINEAR) + resize_bboxes :461-477 on the host
    enhance_lines                       :289-311     cvmi_enhance_lines    (blur -> dilate -> erode, fused, + exact plane sums)
    get_contours                        :388-459     cvmi_external_contours (labelling + border tracing) + the area filter on the host
    contours x component boxes          :1374-1446   cvmi_node_connect     (first near point per (contour, box) + contourMoments' sums)
    valid nodes, ground, renumbering    :1451-1583   assemble_nodes, on the host

The step before it, run_terminal_reclassification (src/analysis_pipeline.py:117-137), rewrites the box list node analysis reads:

    segment_circuit + box emptying      :313-319, :2244-2249   cvmi_segment_circuit   (grey -> 31 x 31 mean -> threshold, fused, + plane sums)
    get_contours(0.0001)                :2254                  cvmi_external_contours + the area filter on the host
    terminal x contour loop             :2272-2286             cvmi_contour_hits      (cvmi_node_connect without broad phase and moments)
    the >= 2 rule and the rewrite       :2288-2308             reclassify_terminals, on the host

A batch stays in HBM until it comes back as contour points (and, for node_connections, the first-hit table and the moment sums).  `contour_img`, the drawing get_contours returns second (drawContours +
putText), is NOT rendered: a zero uint8 [H, W, 3] canvas stands in for it, so that callers that take `.copy()` of it run unchanged.
The same holds for the two drawings get_node_connections adds (:1584-1603).  generate_netlist_from_nodes and what follows stay on the host.
"""
from copy import deepcopy

import numpy as np
import torch

from . import _lib

PRESERVED = ("crossover", "junction", "circuit", "vss")       # circuit_analyzer.py:1332: classes whose boxes stay in the mask
NON_COMPONENTS = ("text", "junction", "crossover", "vss", "explanatory", "circuit")                                   # :51
SOURCE_COMPONENTS = ("voltage.ac", "voltage.dc", "voltage.dependent", "current.dc", "current.dependent")             # :52
SENSITIVE_COMPONENTS = ("diode", "diode.light_emitting", "diode.zener", "transistor.bjt", "transistor.fet")          # :1414
FLT_EPSILON = 1.1920928955078125e-07


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


def contours_packed(planes, shapes, sums=None, binarize=True, cap_contours=None, cap_points=None, keep_device=False):
    """findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) of packed planes (`sums`: the planes' exact sums, int64 device [N], for
    get_contours' inversion; None = no inversion).  binarize: planes that do not invert get the reference's img[img == 255] = 1 in place.
    The first-guess capacities are raised to the true totals and the call repeated when they are short: nothing is truncated.
    keep_device=True: -> (PackedContours, device info i32 [C, 8], device points i32 [P, 2]), what cvmi_node_connect reads."""
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
            pc = PackedContours(np.concatenate((c[:N], c[N + 2:])), info[:nc].cpu().numpy(), area2[:nc].cpu().numpy(),
                                points[:npt].cpu().numpy())
            return (pc, info[:nc], points[:npt]) if keep_device else pc
        cc, cp = max(cc, nc), max(cp, npt)
    raise _lib.CvmiError("external_contours: totals changed between two calls on the same planes")


def contour_dicts(plane_contours, H, W, area_threshold=0.0004, kept=None):
    """get_contours :408-411: contourArea(c) / (H * W) > area_threshold, ids after filtering, boundingRect.
    kept: optional list that receives the positions in `plane_contours` of the contours that pass."""
    norm = H * W
    out = []
    for k, (pts, a2, rect) in enumerate(plane_contours):
        area = abs(a2) / 2.0                                          # contourArea: |shoelace| / 2, exact in double for integer points
        if area / norm > area_threshold:
            out.append({"id": len(out), "contour": np.ascontiguousarray(pts, dtype=np.int32).reshape(-1, 1, 2), "area": area / norm,
                        "rectangle": tuple(int(v) for v in rect)})
            if kept is not None:
                kept.append(k)
    return out


def pixel_threshold(cls):
    """:1407-1415: how near a contour point must come to a box of this class."""
    return 20 if cls in SOURCE_COMPONENTS else (8 if cls in SENSITIVE_COMPONENTS else 6)


def connect_packed(info, points, boxes, box_start, pair_start):
    """cvmi_node_connect on the device outputs of contours_packed(keep_device=True).  boxes: int rows {xmin, ymin, xmax, ymax, threshold}
    of all planes; box_start [N + 1] / pair_start [C + 1]: host offsets (cvmi355.h).
    -> (first i32 [pair_start[C]], moments i64 [C, 3] = {a00, a10, a01}), on the device."""
    lib = _lib.load()
    dev = info.device
    C, P = int(info.shape[0]), int(points.shape[0])
    box_start = np.ascontiguousarray(box_start, dtype=np.int32)
    pair_start = np.ascontiguousarray(pair_start, dtype=np.int32)
    N = len(box_start) - 1
    if len(pair_start) != C + 1:
        raise ValueError(f"pair_start has {len(pair_start)} entries for {C} contours")
    rows = np.asarray(boxes, dtype=np.int64).reshape(-1, 5)
    if len(rows) != int(box_start[-1]):
        raise ValueError(f"{len(rows)} boxes for box offsets that end at {int(box_start[-1])}")
    if len(rows) and np.abs(rows).max() >= 2 ** 30:
        raise ValueError("a box coordinate does not fit the kernel's int32 arithmetic")
    bdev = torch.from_numpy(rows.astype(np.int32)).to(dev) if len(rows) else None
    first = torch.empty(max(int(pair_start[-1]), 1), dtype=torch.int32, device=dev)
    moments = torch.zeros(max(C, 1), 3, dtype=torch.int64, device=dev)
    ws_bytes = int(lib.cvmi_node_connect_workspace(N, C))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.cvmi_node_connect(info.data_ptr(), points.data_ptr(), C, P, bdev.data_ptr() if bdev is not None else None, N,
                                     box_start.ctypes.data, pair_start.ctypes.data, ws.data_ptr(), ws_bytes, first.data_ptr(),
                                     moments.data_ptr(), _stream()), "node_connect")
    return first[:int(pair_start[-1])], moments[:C]


# ---- the host tail of get_node_connections (:1374-1583) -----------------------------------------------------------------------
def moments_from_sums(a00, a10, a01):
    """cv::contourMoments' last step on its three first-order sums, in python floats: m00 = a00 * (+-0.5), m10 / m01 = a * (+-1/6), the
    sign a00's; all zero when |a00| <= FLT_EPSILON.  The sums are exact integers below 2^53, so float() of them is exact."""
    a00, a10, a01 = float(a00), float(a10), float(a01)
    if abs(a00) <= FLT_EPSILON:
        return {"m00": 0.0, "m10": 0.0, "m01": 0.0}
    half, sixth = (0.5, 0.16666666666666666666666666666667) if a00 > 0 else (-0.5, -0.16666666666666666666666666666667)
    return {"m00": a00 * half, "m10": a10 * sixth, "m01": a01 * sixth}


def _component_key(comp):
    uid = comp.get("persistent_uid")
    return uid if uid is not None else (comp["class"], comp["xmin"], comp["ymin"], comp["xmax"], comp["ymax"])


def assemble_nodes(contours, boxes, visited, first, sums):
    """The node list of get_node_connections from the kernel's tables.  contours: get_contours' dicts; boxes: the resized box dicts;
    visited: positions in `boxes` of the boxes the loop visits, in order; first [len(contours), len(visited)]: index of the first near
    point or -1; sums [len(contours), 3]: {a00, a10, a01}.  -> (nodes, connection points)."""
    nodes = {c["id"]: {"id": c["id"], "components": [], "contour": c["contour"]} for c in contours}
    row = {c["id"]: k for k, c in enumerate(contours)}
    points = []
    for j, bi in enumerate(visited):                                  # box-major, contour-minor
        for k, c in enumerate(contours):
            f = int(first[k][j])
            if f < 0:
                continue
            comp = deepcopy(boxes[bi])
            key = _component_key(comp)
            held = nodes[c["id"]]["components"]
            if all(_component_key(e) != key for e in held):           # a duplicate adds neither a component nor a connection point
                held.append(comp)
                points.append(tuple(c["contour"][f][0]))
    valid = {i: n for i, n in nodes.items() if n["components"]}
    if not valid:
        return [], points

    def centroid_y(i):
        m = moments_from_sums(*[int(v) for v in sums[row[i]]])
        return int(m["m01"] / m["m00"]) if m["m00"] != 0 else -float("inf")

    def lowest(ids):                                                  # lowest on screen; the stable sort keeps dict order among ties
        return sorted(ids, key=centroid_y, reverse=True)[0]
    most = max(len(n["components"]) for n in valid.values())
    with_source = [i for i, n in valid.items() if any(c["class"] in SOURCE_COMPONENTS for c in n["components"])]
    with_most = [i for i, n in valid.items() if len(n["components"]) == most]
    ground = lowest(with_source) if with_source else (lowest(with_most) if with_most else lowest(list(valid)))
    out = []
    if ground is not None and ground in valid:
        out.append({"id": 0, "components": valid[ground]["components"], "contour": valid[ground]["contour"]})
        for i in sorted(i for i in valid if i != ground):
            n = valid[i]
            if len(n["components"]) >= 2 or (len(out) == 1 and len(valid) == 2):
                out.append({"id": len(out), "components": n["components"], "contour": n["contour"]})
    else:                                                             # no ground: number the valid nodes as they come
        for i in sorted(valid):
            out.append({"id": len(out), "components": valid[i]["components"], "contour": valid[i]["contour"]})
    return out, points


# ---- terminal reclassification (circuit_analyzer.py:2217-2311) ----------------------------------------------------------------
RECLASS_NEAR = 10                                                     # pixel_threshold_for_reclass :2277
RECLASS_AREA = 0.0001                                                 # get_contours' threshold at :2254


def emptying_rects(bboxes, H, W):
    """:2244-2249 as plain rectangles: numpy resolves mask[max(0, ymin):min(H, ymax), max(0, xmin):min(W, xmax)] -- without a ymin < ymax
    guard a negative ymax / xmax counts from the end -- so slice.indices gives the rows and columns it writes.  -> [[x0, y0, x1, y1]],
    half-open, non-empty."""
    out = []
    for b in bboxes:
        if b.get("class") in PRESERVED:
            continue
        y0, y1, _ = slice(max(0, int(b["ymin"])), min(H, int(b["ymax"]))).indices(H)
        x0, x1, _ = slice(max(0, int(b["xmin"])), min(W, int(b["xmax"]))).indices(W)
        if y0 < y1 and x0 < x1:
            out.append([x0, y0, x1, y1])
    return out


def segment_packed(src, planes, rects, red_channel=0):
    """cvmi_segment_circuit.  src: a flat u8 device buffer; planes: [(byte offset, pitch in bytes, H, W)] windows of u8 [., ., 3] images in
    it; rects: per plane [[x0, y0, x1, y1]] (emptying_rects).  -> (packed u8 masks, exact plane sums as int64 [N]), on the device."""
    lib = _lib.load()
    N = len(planes)
    geom = np.ascontiguousarray(np.asarray(planes, dtype=np.int64).reshape(N, 4))
    start = np.concatenate(([0], np.cumsum([len(r) for r in rects]))).astype(np.int32)
    rows = [r for rr in rects for r in rr]
    rdev = torch.tensor(rows, dtype=torch.int32).reshape(-1, 4).to(src.device) if rows else None
    dst = torch.empty(int((geom[:, 2] * geom[:, 3]).sum()), dtype=torch.uint8, device=src.device)
    sums = torch.empty(N, dtype=torch.int64, device=src.device)
    _lib.check(lib.cvmi_segment_circuit(src.data_ptr(), src.numel(), N, geom.ctypes.data, int(red_channel), rdev.data_ptr() if rdev is not None else None,
                                        start.ctypes.data, dst.data_ptr(), sums.data_ptr(), _stream()), "segment_circuit")
    return dst, sums


def hits_packed(info, points, boxes, box_start, pair_start):
    """cvmi_contour_hits on the device outputs of contours_packed(keep_device=True): connect_packed without the broad phase and the
    moments.  -> first i32 [pair_start[C]] on the device."""
    lib = _lib.load()
    dev = info.device
    C, P = int(info.shape[0]), int(points.shape[0])
    box_start = np.ascontiguousarray(box_start, dtype=np.int32)
    pair_start = np.ascontiguousarray(pair_start, dtype=np.int32)
    N = len(box_start) - 1
    if len(pair_start) != C + 1:
        raise ValueError(f"pair_start has {len(pair_start)} entries for {C} contours")
    rows = np.asarray(boxes, dtype=np.int64).reshape(-1, 5)
    if len(rows) != int(box_start[-1]):
        raise ValueError(f"{len(rows)} boxes for box offsets that end at {int(box_start[-1])}")
    if len(rows) and np.abs(rows).max() >= 2 ** 30:
        raise ValueError("a box coordinate does not fit the kernel's int32 arithmetic")
    bdev = torch.from_numpy(rows.astype(np.int32)).to(dev) if len(rows) else None
    first = torch.empty(max(int(pair_start[-1]), 1), dtype=torch.int32, device=dev)
    ws_bytes = int(lib.cvmi_contour_hits_workspace(N, C))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.cvmi_contour_hits(info.data_ptr(), points.data_ptr(), C, P, bdev.data_ptr() if bdev is not None else None, N,
                                     box_start.ctypes.data, pair_start.ctypes.data, ws.data_ptr(), ws_bytes, first.data_ptr(), _stream()), "contour_hits")
    return first[:int(pair_start[-1])]


def _rgb_planes(images, windows):
    """-> (flat u8 device buffer, [(byte offset, pitch, H, W)])."""
    if windows is not None and hasattr(images, "offsets"):            # rectangles of the images of a detector.PackedImages, read in place
        if not images.data.is_cuda or len(windows) != len(images):
            raise ValueError("with windows, a PackedImages is on the device and windows has one entry per image")
        planes = []
        for b, (w, (H, W), off) in enumerate(zip(windows, images.shapes, images.offsets)):
            x0, y0, x1, y1 = (0, 0, W, H) if w is None else (int(v) for v in w)
            if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
                raise ValueError(f"window {b} = {w} leaves the {H} x {W} image")
            planes.append((off + y0 * W * 3 + x0 * 3, W * 3, y1 - y0, x1 - x0))
        return images.data, planes
    if windows is not None:                                           # rectangles of one u8 [B, H, W, 3] device block, read in place
        if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_cuda \
                or not images.is_contiguous() or len(windows) != images.shape[0]:
            raise ValueError("with windows, images is one contiguous uint8 [B, H, W, 3] device block and windows has B entries")
        _, H, W, _ = images.shape
        planes = []
        for b, w in enumerate(windows):
            x0, y0, x1, y1 = (0, 0, W, H) if w is None else (int(v) for v in w)
            if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
                raise ValueError(f"window {b} = {w} leaves the {H} x {W} image")
            planes.append(((b * H + y0) * W * 3 + x0 * 3, W * 3, y1 - y0, x1 - x0))
        return images.view(-1), planes
    flat, planes, off = [], [], 0
    for im in images:
        if isinstance(im, np.ndarray):
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError(f"expected a uint8 [H, W, 3] image, got {im.dtype} {im.shape}")
            im = torch.from_numpy(np.ascontiguousarray(im)).to(_dev())
        elif not torch.is_tensor(im) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or not im.is_cuda:
            raise ValueError("expected a uint8 [H, W, 3] numpy image or device tensor")
        H, W = int(im.shape[0]), int(im.shape[1])
        flat.append(im.contiguous().view(-1))
        planes.append((off, W * 3, H, W))
        off += H * W * 3
    return (flat[0] if len(flat) == 1 else torch.cat(flat)), planes


def _dc_id(names):
    for num_id, name in (names.items() if hasattr(names, "items") else enumerate(names)):      # :2263-2267
        if name == "voltage.dc":
            return num_id
    return None


def reclassify_terminals(images, bboxes, names, red_channel=0, windows=None, events=None):
    """reclassify_terminals_based_on_connectivity (circuit_analyzer.py:2229-2308) for a batch.  images: u8 [H_i, W_i, 3] device tensors
    or numpy arrays, or -- with windows = [(x0, y0, x1, y1) | None] -- one u8 [B, H, W, 3] device block, or a `detector.PackedImages`
    (images of different sizes in one buffer), whose rectangles are the planes (read in place).  red_channel: the channel of `images` that takes cvtColor(RGB2GRAY)'s R weight: 0 for the image
    run_terminal_reclassification is handed (it swaps, and the method swaps back), 2 for the method's own argument.
    names: the detector's {id: name} (self.yolo.model.names).  Only images with a 'terminal' box are processed: segment + empty
    (cvmi_segment_circuit), contours, the hit table, then the host rule.  The box dicts are rewritten IN PLACE (:2297-2308).
    -> per image {box index: number of connected contours} for its terminals.
    A terminal's coordinates must be integral-valued (the pipeline's are): the kernel tests in integers.
    events: optional list that receives (name, torch.cuda.Event) pairs around the sub-stages (tools/terminal_reclass_bench.py)."""
    n_img = len(windows) if windows is not None else len(images)
    if len(bboxes) != n_img:
        raise ValueError(f"{len(bboxes)} box lists for {n_img} images")
    out = [{} for _ in range(n_img)]
    terms = [[k for k, b in enumerate(bb) if b.get("class") == "terminal"] for bb in bboxes]
    for bb, tk in zip(bboxes, terms):
        for k in tk:
            for key in ("xmin", "ymin", "xmax", "ymax"):
                if bb[k][key] != int(bb[k][key]):
                    raise ValueError(f"terminal box {k} has {key} = {bb[k][key]!r}: the device test needs integral-valued coordinates")
    sel = [i for i in range(n_img) if terms[i]]
    if not sel:
        return out

    def mark(name):
        if events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events.append((name, e))
    if windows is not None:
        src, planes = _rgb_planes(images, windows)
        planes = [planes[i] for i in sel]
    else:
        src, planes = _rgb_planes([images[i] for i in sel], None)
    shapes = [(h, w) for _, _, h, w in planes]
    mark("start")
    masks, sums = segment_packed(src, planes, [emptying_rects(bboxes[i], h, w) for i, (h, w) in zip(sel, shapes)], red_channel)
    mark("segment")
    pc, info_dev, points_dev = contours_packed(masks, shapes, sums, binarize=True, keep_device=True)
    mark("contours")
    rows = [[int(bboxes[i][k]["xmin"]), int(bboxes[i][k]["ymin"]), int(bboxes[i][k]["xmax"]), int(bboxes[i][k]["ymax"]), RECLASS_NEAR] for i in sel for k in terms[i]]
    box_start = np.concatenate(([0], np.cumsum([len(terms[i]) for i in sel]))).astype(np.int32)
    per_plane = np.asarray(pc.counts[:len(sel)], dtype=np.int64)
    pair_start = np.concatenate(([0], np.cumsum(np.repeat(np.diff(box_start), per_plane)))).astype(np.int64)
    if pair_start[-1] >= 2 ** 31:
        raise ValueError(f"{int(pair_start[-1])} (contour, box) pairs exceed the int32 offsets")
    first = hits_packed(info_dev, points_dev, rows, box_start, pair_start)
    mark("hits")
    first = first.cpu().numpy()
    dc = _dc_id(names)
    c0 = 0
    for j, i in enumerate(sel):
        h, w = shapes[j]
        kept = []
        contour_dicts(pc.plane(j), h, w, RECLASS_AREA, kept)          # get_contours' area filter :410
        nb = len(terms[i])
        hit = np.zeros(nb, dtype=np.int64)
        for k in kept:
            hit += first[pair_start[c0 + k]:pair_start[c0 + k] + nb] >= 0
        c0 += int(pc.counts[j])
        for t, k in enumerate(terms[i]):
            out[i][k] = int(hit[t])
            if hit[t] >= 2:                                           # :2293-2308
                b = bboxes[i][k]
                b["original_yolo_class_if_reclassified"] = b["class"]
                b["class"] = "voltage.dc"
                if dc is not None:
                    b["_yolo_class_id_temp"] = dc
                b["was_reclassified_from_terminal"] = True
    return out


def segment_circuit(img):
    """CircuitAnalyzer.segment_circuit (circuit_analyzer.py:313-319) on a u8 [H, W, 3] numpy image (-> numpy) or device tensor (-> tensor):
    cvtColor(RGB2GRAY), the R weight on channel 0, then adaptiveThreshold(255, MEAN_C, BINARY_INV, 31, 21).  -> u8 [H, W], 0 / 255."""
    src, planes = _rgb_planes([img], None)
    masks, _ = segment_packed(src, planes, [[]], 0)
    m = masks.view(planes[0][2], planes[0][3])
    return m.cpu().numpy() if isinstance(img, np.ndarray) else m


def reclassify_terminals_based_on_connectivity(image_rgb_original, bboxes_list_to_modify, names):
    """CircuitAnalyzer.reclassify_terminals_based_on_connectivity (circuit_analyzer.py:2217-2311): the method's cvtColor(RGB2BGR) in front of
    segment_circuit puts the R weight on channel 2 of its argument.  `names` stands for self.yolo.model.names.  Rewrites the list's dicts in
    place and returns None, as the reference does."""
    reclassify_terminals([image_rgb_original], [bboxes_list_to_modify], names, red_channel=2)


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


def _resized_boxes(bb, h, w, nh, nw):
    """resize_bboxes :461-477."""
    sx, sy = nw / w, nh / h
    out = []
    for b in bb:
        r = dict(b)
        r["xmin"], r["ymin"], r["xmax"], r["ymax"] = int(b["xmin"] * sx), int(b["ymin"] * sy), int(b["xmax"] * sx), int(b["ymax"] * sy)
        out.append(r)
    return out


def _node_front(masks, bboxes, new_height, area_threshold, events, connect):
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
    if connect:
        pc, info_dev, points_dev = contours_packed(enhanced, new_shapes, sums, binarize=True, keep_device=True)
    else:
        pc = contours_packed(enhanced, new_shapes, sums, binarize=True)
    mark("contours")
    rbs = [_resized_boxes(bb, h, w, nh, nw) for bb, (h, w), (nh, nw) in zip(bboxes, shapes, new_shapes)]
    if connect:                                                       # all contours of the batch against their planes' boxes, one launch
        visited = [[k for k, b in enumerate(rb) if b["class"] not in NON_COMPONENTS] for rb in rbs]
        rows = [[rb[k]["xmin"], rb[k]["ymin"], rb[k]["xmax"], rb[k]["ymax"], pixel_threshold(rb[k]["class"])] for rb, v in zip(rbs, visited) for k in v]
        box_start = np.concatenate(([0], np.cumsum([len(v) for v in visited]))).astype(np.int32)
        per_plane = np.asarray(pc.counts[:len(shapes)], dtype=np.int64)
        pair_start = np.concatenate(([0], np.cumsum(np.repeat(np.diff(box_start), per_plane)))).astype(np.int64)
        if pair_start[-1] >= 2 ** 31:
            raise ValueError(f"{int(pair_start[-1])} (contour, box) pairs exceed the int32 offsets")
        first_dev, mom_dev = connect_packed(info_dev, points_dev, rows, box_start, pair_start)
        mark("connect")
        first, mom = first_dev.cpu().numpy(), mom_dev.cpu().numpy()
    roffs = np.concatenate(([0], np.cumsum([h * w for h, w in new_shapes], dtype=np.int64)))
    em, en = _views(emptied, offs, shapes), _views(enhanced, roffs, new_shapes)
    out, c0 = [], 0
    for i, (nh, nw) in enumerate(new_shapes):
        kept = []
        r = {"emptied_mask": em[i], "resized_bboxes": rbs[i], "enhanced": en[i],
             "contours": contour_dicts(pc.plane(i), nh, nw, area_threshold, kept)}
        if connect:                                                   # the rows of the contours that pass the area filter
            nb = len(visited[i])
            f = [first[pair_start[c0 + k]:pair_start[c0 + k] + nb] for k in kept]
            r["nodes"], r["connection_points"] = assemble_nodes(r["contours"], rbs[i], visited[i], f, [mom[c0 + k] for k in kept])
            c0 += int(pc.counts[i])
        out.append(r)
    if events is not None:
        events.append(("longest_border", pc.longest_border))
    return out


def node_contours(masks, bboxes, new_height=600, area_threshold=0.0004, events=None):
    """get_node_connections up to get_contours (circuit_analyzer.py:1325-1365) for a batch of u8 device masks [H_i, W_i] and their
    crop-relative boxes, in three launches over all planes.  -> per image {"emptied_mask": u8 [H, W] device (before the resize),
    "resized_bboxes": resize_bboxes' dicts, "enhanced": u8 [new_height, new_w] device as the reference leaves `enhanced` after
    get_contours (255 -> 1 where the plane did not invert), "contours": get_contours' dicts}.
    events: optional list that receives (name, torch.cuda.Event) pairs around the sub-stages (tools/node_stage_bench.py)."""
    if not masks:
        return []
    return _node_front(masks, bboxes, new_height, area_threshold, events, False)


def node_connections(masks, bboxes, new_height=600, area_threshold=0.0004, events=None):
    """get_node_connections up to its node list (circuit_analyzer.py:1325-1583) for a batch: node_contours, then every contour of the
    batch against the component boxes of its plane in one more launch (cvmi_node_connect), then the host tail (assemble_nodes).
    -> node_contours' dicts plus "nodes": [{"id", "components": deep copies of the resized box dicts, "contour"}], ground = id 0, and
    "connection_points": the (x, y) the reference only draws, in the order it finds them.
    events: as node_contours, with a "connect" mark after the extra launch (tools/node_connect_bench.py)."""
    if not masks:
        return []
    return _node_front(masks, bboxes, new_height, area_threshold, events, True)


def get_node_connections(image_for_context, processing_wire_mask, bboxes_relative_to_mask):
    """CircuitAnalyzer.get_node_connections (circuit_analyzer.py:1286-1605), same arguments and six-tuple:
    -> (new_nodes_list, emptied_mask, enhanced, contour_img, final_viz, connection_points_viz).  The mask is a u8 [H, W] numpy plane (the
    two planes come back as numpy) or device tensor (they stay on the device).  The three drawings are NOT rendered: zero uint8
    [new_height, new_w, 3] canvases of the reference's shapes stand in (wires.node_connections gives the connection points as data).
    A None mask returns ([], canvas x 5) with the canvas sized by the context image, or 100 x 100 without one, as the reference does."""
    if processing_wire_mask is None:
        h, w = image_for_context.shape[:2] if image_for_context is not None else (100, 100)
        blank = np.zeros((h, w, 3), dtype=np.uint8)
        return [], blank, blank, blank, blank, blank
    x, was_np = _to_device_u8(processing_wire_mask)
    r = node_connections([x], [bboxes_relative_to_mask])[0]
    emptied, enhanced = r["emptied_mask"], r["enhanced"]
    nh, nw = enhanced.shape
    if was_np:
        emptied, enhanced = emptied.cpu().numpy(), enhanced.cpu().numpy()
    canvas = lambda: np.zeros((nh, nw, 3), dtype=np.uint8)            # noqa: E731
    return r["nodes"], emptied, enhanced, canvas(), canvas(), canvas()
