"""Node-analysis front end on the device: the step that consumes the segmenter's mask.

What it restates is the start of CircuitAnalyzer.get_node_connections (/root/reference/src/circuit_analyzer.py:1286-1370), which the
reference runs per image on the host through OpenCV (run_node_analysis, src/analysis_pipeline.py:227):

    empty the component boxes           :1327-1345   cvmi_node_prepare     (wire_ops.hip)
    resize_image_keep_aspect(600)       :787-809     cvmi_node_prepare     (cv2.resize INTER_LINEAR) + resize_bboxes :461-477 on the host
    enhance_lines                       :289-311     cvmi_enhance_lines    (blur -> dilate -> erode, fused, + exact plane sums)
    get_contours                        :388-459     cvmi_external_contours (labelling + border tracing) + the area filter on the host
    contours x component boxes          :1374-1446   cvmi_node_connect     (first near point per (contour, box) + contourMoments' sums)
    valid nodes, ground, renumbering    :1451-1583   assemble_nodes, on the host

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
