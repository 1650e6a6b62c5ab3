"""Plain-Python restatement of the tail of the reference's get_node_connections and of OpenCV's contourMoments.  TEST INFRASTRUCTURE ONLY
(slow: every box x every contour x every contour point, interpreted).  Built on tests/wire_ref.py, which restates the front end.

CircuitAnalyzer.get_node_connections (circuit_analyzer.py:1374-1583), after get_contours:
  1. every box whose class is a component (not in non_components, :51), in list order, against every contour in list order:
     broad phase :1399-1401 (box against the contour's boundingRect, closed, no threshold), then the contour's points in order until the
     first that passes is_point_near_bbox :811-846 (inside the closed box, or within the class threshold :1407-1415 of one of the four
     edge LINES); that point is a connection point and the box (a deep copy of the RESIZED dict) a component of the contour's node,
     unless the node already holds a component with the same persistent_uid (or the same class + coordinates when there is no uid)
  2. valid nodes = nodes with a component; ground = of the source-connected nodes the lowest on screen (int(m01 / m00) of
     cv2.moments, -inf when m00 == 0), else of the nodes with the most components, else of all valid nodes; ties keep dict order
  3. ground becomes id 0, the others follow in ascending old id when they have >= 2 components (or when there are exactly two valid
     nodes)

[UP] (unpinned: OpenCV is not installed) contourMoments, modules/imgproc/src/moments.cpp: with (x_prev, y_prev) starting at the LAST point,
dxy = x_prev y - x y_prev; a00 += dxy; a10 += dxy (x_prev + x); a01 += dxy (y_prev + y), in doubles (exact while below 2^53); then
m00 = a00 * (+-0.5), m10 = a10 * (+-1/6), m01 = a01 * (+-1/6) with a00's sign, all zero when |a00| <= FLT_EPSILON.
"""
from copy import deepcopy

import numpy as np

import wire_ref as W

NON_COMPONENTS = {"text", "junction", "crossover", "vss", "explanatory", "circuit"}
SOURCE_COMPONENTS = {"voltage.ac", "voltage.dc", "voltage.dependent", "current.dc", "current.dependent"}
SENSITIVE = ("diode", "diode.light_emitting", "diode.zener", "transistor.bjt", "transistor.fet")
FLT_EPSILON = 2.0 ** -23


def threshold_of(cls):
    if cls in SOURCE_COMPONENTS:
        return 20
    return 8 if cls in SENSITIVE else 6


def is_point_near_bbox(point, bbox, t):
    px, py = int(point[0]), int(point[1])
    if bbox["xmin"] <= px <= bbox["xmax"] and bbox["ymin"] <= py <= bbox["ymax"]:
        return True
    return min(abs(px - bbox["xmin"]), abs(px - bbox["xmax"]), abs(py - bbox["ymin"]), abs(py - bbox["ymax"])) <= t


def broad_phase_skips(bbox, rect):
    x, y, w, h = rect
    return bbox["xmax"] < x or bbox["xmin"] > x + w or bbox["ymax"] < y or bbox["ymin"] > y + h


def first_near(pts, rect, bbox, t):
    """Index of the first of `pts` [(x, y)] near the box, -1 when there is none or the broad phase skips the pair."""
    if broad_phase_skips(bbox, rect):
        return -1
    for i, p in enumerate(pts):
        if is_point_near_bbox(p, bbox, t):
            return i
    return -1


def _points(contour):
    return [(int(p[0]), int(p[1])) for p in np.asarray(contour).reshape(-1, 2)]


def contour_sums(contour):
    """[UP] (a00, a10, a01) of contourMoments as python ints."""
    pts = _points(contour)
    a00 = a10 = a01 = 0
    if not pts:
        return 0, 0, 0
    xp, yp = pts[-1]
    for x, y in pts:
        dxy = xp * y - x * yp
        a00 += dxy
        a10 += dxy * (xp + x)
        a01 += dxy * (yp + y)
        xp, yp = x, y
    return a00, a10, a01


def moments(contour):
    """[UP] cv2.moments(contour)'s m00, m10, m01 (the keys get_node_connections reads)."""
    a00, a10, a01 = (float(v) for v in contour_sums(contour))
    if abs(a00) <= FLT_EPSILON:
        return {"m00": 0.0, "m10": 0.0, "m01": 0.0}
    s = 1.0 if a00 > 0 else -1.0
    return {"m00": a00 * (s * 0.5), "m10": a10 * (s * 0.16666666666666666666666666666667), "m01": a01 * (s * 0.16666666666666666666666666666667)}


def centroid_y(contour):
    m = moments(contour)
    return int(m["m01"] / m["m00"]) if m["m00"] != 0 else -float("inf")


def _ref_of(comp):
    uid = comp.get("persistent_uid")
    return uid if uid is not None else (comp["class"], comp["xmin"], comp["ymin"], comp["xmax"], comp["ymax"])


def node_tail(contours, resized_bboxes):
    """Steps 1-3 above: -> (node list, connection points)."""
    nodes = {c["id"]: {"id": c["id"], "components": [], "contour": c["contour"]} for c in contours}
    conn = []
    for bbox in resized_bboxes:
        if bbox["class"] in NON_COMPONENTS:
            continue
        t = threshold_of(bbox["class"])
        for c in contours:
            pts = _points(c["contour"])
            i = first_near(pts, c["rectangle"], bbox, t)
            if i < 0:
                continue
            comp = deepcopy(bbox)
            if _ref_of(comp) not in [_ref_of(e) for e in nodes[c["id"]]["components"]]:
                nodes[c["id"]]["components"].append(comp)
                conn.append(pts[i])
    valid = {k: v for k, v in nodes.items() if v["components"]}
    if not valid:
        return [], conn
    cy = {c["id"]: centroid_y(c["contour"]) for c in contours if c["id"] in valid}
    most = max(len(v["components"]) for v in valid.values())
    tiers = ([k for k, v in valid.items() if any(e["class"] in SOURCE_COMPONENTS for e in v["components"])],
             [k for k, v in valid.items() if len(v["components"]) == most], list(valid))
    cands = next(t for t in tiers if t)
    ground = cands[0]
    for k in cands[1:]:                                               # the first of the largest centroid_y: a stable descending sort's head
        if cy[k] > cy[ground]:
            ground = k
    out = [{"id": 0, "components": valid[ground]["components"], "contour": valid[ground]["contour"]}]
    for k in sorted(valid):
        if k != ground and (len(valid[k]["components"]) >= 2 or len(valid) == 2):
            out.append({"id": len(out), "components": valid[k]["components"], "contour": valid[k]["contour"]})
    return out, conn


def node_connections(mask, bboxes, new_height=600, area_threshold=0.0004):
    """One image through wire_ref's front end and node_tail: the dict circuitvision_amd.wires.node_connections gives per image."""
    emptied, rb, enhanced, contours = W.node_contours(mask, bboxes, new_height, area_threshold)
    nodes, conn = node_tail(contours, rb)
    return {"emptied_mask": emptied, "resized_bboxes": rb, "enhanced": enhanced, "contours": contours, "nodes": nodes, "connection_points": conn}


def get_node_connections(image_for_context, mask, bboxes):
    """The reference's six-tuple, the drawings as zero canvases of its shapes."""
    if mask is None:
        h, w = image_for_context.shape[:2] if image_for_context is not None else (100, 100)
        blank = np.zeros((h, w, 3), np.uint8)
        return [], blank, blank, blank, blank, blank
    r = node_connections(mask, bboxes)
    h, w = r["enhanced"].shape
    return (r["nodes"], r["emptied_mask"], r["enhanced"]) + tuple(np.zeros((h, w, 3), np.uint8) for _ in range(3))


# ---- the fixture's vocabulary (tests/golden/node_connections.json) -----------------------------------------------------------------
def rails(h, w, seed):
    """Rows [(y0, y1)] and columns (x0, x1) of the horizontal wires of rails_mask: 2 + seed % 3 rails, 4 + (seed // 3) % 3 pixels thick."""
    k, th = 2 + seed % 3, 4 + (seed // 3) % 3
    return [((i + 1) * h // (k + 1), (i + 1) * h // (k + 1) + th) for i in range(k)], (w // 10 + seed % 5, w - w // 10 - seed % 7)


def rails_mask(h, w, seed):
    """A 0 / 255 mask of parallel horizontal wires: every rail is one contour, so a test can say which boxes touch which node."""
    m = np.zeros((h, w), np.uint8)
    rows, (x0, x1) = rails(h, w, seed)
    for y0, y1 in rows:
        m[y0:y1, x0:x1] = 255
    return m


def golden_mask(spec):
    if spec is None:
        return None
    if spec["gen"] == "rails":
        return rails_mask(spec["h"], spec["w"], spec["seed"])
    from synth import circuit_image
    return W.wire_mask(circuit_image(spec["h"], spec["w"], seed=spec["seed"]))


def points_checksum(contour):
    """Order-sensitive checksum of a contour's points."""
    s = 0
    for i, (x, y) in enumerate(_points(contour)):
        s = (s * 1000003 + (i + 1) * (x * 4099 + y)) % (2 ** 61 - 1)
    return s


def summarize(result):
    """What the fixture records of a six-tuple (plus the connection points, which the reference only draws)."""
    nodes, conn = result[0], result[6] if len(result) > 6 else None
    out = {"nodes": [{"id": int(n["id"]), "uids": [c.get("persistent_uid") for c in n["components"]], "classes": [c["class"] for c in n["components"]],
                      "coords": [[int(c[k]) for k in ("xmin", "ymin", "xmax", "ymax")] for c in n["components"]],
                      "npts": int(len(n["contour"])), "checksum": points_checksum(n["contour"])} for n in nodes],
           "shapes": [list(a.shape) for a in result[1:6]]}
    if conn is not None:
        out["connection_points"] = [[int(p[0]), int(p[1])] for p in conn]
    return out
