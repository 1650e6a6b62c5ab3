"""get_node_connections on the GPU (cvmi_node_connect via circuitvision_amd.wires) against tests/node_ref.py, bit for bit: the first-hit
table and the moment sums at op level (chunk seams, the broad phase, more boxes than one LDS tile), the batched node list, the
reference-shaped wrapper and the pipeline switch."""
import numpy as np
import pytest
import torch

import node_ref as R
import wire_ref as W
from circuitvision_amd import wires
from synth import circuit_image

pytestmark = pytest.mark.gpu

CHUNK = 1024                                                           # NC_CHUNK of wire_ops.hip: contour points per workgroup
BOX_TILE = 256                                                         # NC_BOX_TILE: boxes in LDS at a time


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _wire(h, w, seed):
    return W.wire_mask(circuit_image(h, w, seed=seed))


def _connect(planes, rows_per_plane):
    """Contours of raw 0 / 255 planes (no inversion) and the connect op on them.  rows: [xmin, ymin, xmax, ymax, t] per box.
    -> per plane [(points, rect, first row, sums)] from the device, and the host copy of the contours."""
    shapes = [p.shape for p in planes]
    buf = torch.cat([_dev(p).reshape(-1) for p in planes])
    pc, info, points = wires.contours_packed(buf, shapes, None, binarize=False, keep_device=True)
    box_start = np.concatenate(([0], np.cumsum([len(r) for r in rows_per_plane]))).astype(np.int32)
    per_plane = np.asarray(pc.counts[:len(planes)], dtype=np.int64)
    pair_start = np.concatenate(([0], np.cumsum(np.repeat(np.diff(box_start), per_plane))))
    first, mom = wires.connect_packed(info, points, [r for rows in rows_per_plane for r in rows], box_start, pair_start)
    assert first.dtype == torch.int32 and mom.dtype == torch.int64 and tuple(mom.shape) == (int(per_plane.sum()), 3)
    first, mom = first.cpu().numpy(), mom.cpu().numpy()
    out, c = [], 0
    for n, rows in enumerate(rows_per_plane):
        got = []
        for pts, _a2, rect in pc.plane(n):
            got.append(([tuple(v) for v in pts.tolist()], tuple(rect), first[pair_start[c]:pair_start[c + 1]].tolist(), tuple(mom[c].tolist())))
            c += 1
        out.append(got)
    assert c == len(pair_start) - 1
    return out


def _box(r):
    return {"xmin": r[0], "ymin": r[1], "xmax": r[2], "ymax": r[3]}


def _assert_matches_ref(plane_result, rows, what=""):
    for k, (pts, rect, first, sums) in enumerate(plane_result):
        want = [R.first_near(pts, rect, _box(r), r[4]) for r in rows]
        assert first == want, (what, k, first, want)
        assert sums == R.contour_sums(pts), (what, k)


def _rand_rows(rng, n, h, w):
    rows = []
    for _ in range(n):
        x, y = int(rng.integers(-10, w)), int(rng.integers(-10, h))
        rows.append([x, y, x + int(rng.integers(0, 40)), y + int(rng.integers(0, 40)), int(rng.choice([6, 8, 20]))])
    return rows


def comb(h=40, w=640):
    """A spine with one-pixel teeth on both sides: CHAIN_APPROX_SIMPLE keeps several points per tooth, so the border is long."""
    m = np.zeros((h, w), np.uint8)
    m[18:22, 2:w - 2] = 255
    m[14:18, 2:w - 2:2] = 255
    m[22:26, 3:w - 2:2] = 255
    return m


# ---- op level -------------------------------------------------------------------------------------------------------------------------
def test_first_and_moments_on_packed_planes_with_an_empty_plane_and_a_plane_without_boxes():
    rng = np.random.default_rng(0)
    planes = [_wire(120, 160, 11), np.zeros((50, 70), np.uint8), np.where(rng.random((97, 131)) < 0.3, 255, 0).astype(np.uint8), _wire(101, 143, 12)]
    rows = [_rand_rows(rng, 7, 120, 160), _rand_rows(rng, 2, 50, 70), [], _rand_rows(rng, 5, 101, 143)]
    got = _connect(planes, rows)
    assert len(got[0]) > 1 and got[1] == [] and len(got[2]) > 1 and len(got[3]) > 1
    for n, p in enumerate(planes):                                      # the contours themselves are wire_ref's
        assert [g[0] for g in got[n]] == W.find_external_contours(p != 0), n
        _assert_matches_ref(got[n], rows[n], n)
    assert all(g[2] == [] for g in got[2])
    assert any(f >= 0 for g in got[0] + got[3] for f in g[2]) and any(f < 0 for g in got[0] + got[3] for f in g[2])


def test_a_contour_of_several_chunks_lowest_index_wins_and_the_ends_are_found():
    m = comb()
    pts = W.find_external_contours(m != 0)
    assert len(pts) == 1 and len(pts[0]) > 2 * CHUNK
    pts = pts[0]
    n = len(pts)
    assert pts.count(pts[0]) == 1 and pts.count(pts[-1]) == 1
    seam = pts[2 * CHUNK]
    rows = [[300, 0, 330, 39, 6],                                       # a band across the spine: near points on the way out and on the way back
            [pts[-1][0], pts[-1][1], pts[-1][0], pts[-1][1], -1],       # t = -1: no edge line counts, only the box's one pixel = the LAST point
            [pts[0][0], pts[0][1], pts[0][0], pts[0][1], -1],           # ... = point 0
            [seam[0], seam[1], seam[0], seam[1], -1],                   # the first point of the third chunk
            [0, 0, 639, 39, 6],                                         # everything is inside: 0
            [pts[CHUNK - 1][0], pts[CHUNK - 1][1], pts[CHUNK - 1][0], pts[CHUNK - 1][1], -1]]      # the last point of the first chunk
    got = _connect([m], [rows])[0]
    assert len(got) == 1 and got[0][0] == pts
    _assert_matches_ref(got, rows)
    first = got[0][2]
    hits = [i for i, p in enumerate(pts) if R.is_point_near_bbox(p, _box(rows[0]), 6)]
    assert len({i // CHUNK for i in hits}) >= 2 and first[0] == hits[0]  # near points in different chunks
    assert first[1] == n - 1 and (n - 1) // CHUNK >= 2 and first[2] == 0 and first[4] == 0
    assert first[3] == pts.index(seam) and first[5] == pts.index(pts[CHUNK - 1])


def test_moments_across_chunk_seams_and_on_contours_of_one_two_and_three_points():
    t = np.zeros((20, 30), np.uint8)
    t[2, 2] = 255                                                       # 1 point
    t[5, 5:7] = 255                                                     # 2 points
    t[10, 10] = t[10, 11] = t[11, 10] = 255                             # 3 points
    got = _connect([comb(), t, comb(44, 1100).T.copy()], [[], [[0, 0, 5, 5, 6]], []])
    assert sorted(len(g[0]) for g in got[1]) == [1, 2, 3]
    assert len(got[0][0][0]) > 2 * CHUNK and len(got[2][0][0]) > 4 * CHUNK
    for n in range(3):
        for pts, _rect, _first, sums in got[n]:
            assert sums == R.contour_sums(pts), (n, len(pts))
    assert got[0][0][3][0] != 0 and [g[3][0] for g in got[1] if len(g[0]) < 3] == [0, 0]


def test_broad_phase_has_no_threshold():
    m = np.zeros((60, 80), np.uint8)
    m[20:40, 10:50] = 255                                               # rectangle (10, 20, 40, 20): x + w = 50
    rows = [[53, 25, 70, 35, 6], [50, 25, 70, 35, 6], [51, 25, 70, 35, 6], [20, 44, 30, 50, 6], [20, 40, 30, 50, 6], [0, 0, 9, 19, 20], [0, 0, 10, 20, 20]]
    got = _connect([m], [rows])[0]
    pts, rect, first, _ = got[0]
    assert rect == (10, 20, 40, 20)
    assert any(R.is_point_near_bbox(p, _box(rows[0]), 6) for p in pts) and first[0] == -1      # 3 px clear of the rectangle, points within 6
    assert first[1] >= 0 and first[2] == -1 and first[3] == -1 and first[4] >= 0 and first[5] == -1 and first[6] >= 0
    _assert_matches_ref(got, rows)


def test_more_boxes_on_a_plane_than_one_lds_tile():
    rng = np.random.default_rng(3)
    planes = [_wire(96, 128, 21), _wire(110, 90, 22)]
    rows = [_rand_rows(rng, 2 * BOX_TILE + 37, 96, 128), _rand_rows(rng, 3, 110, 90)]
    got = _connect(planes, rows)
    for n in range(2):
        _assert_matches_ref(got[n], rows[n], n)
    tail = [g[2][BOX_TILE:] for g in got[0]]
    assert any(f >= 0 for r in tail for f in r)


# ---- the node list --------------------------------------------------------------------------------------------------------------------
CLASSES = ["voltage.dc", "resistor", "transistor.bjt", "capacitor.unpolarized", "text", "diode", "gnd", "crossover", "current.dc", "inductor", "junction"]


def _boxes(rng, h, w, n):
    bb = []
    for k in range(n):
        x, y = float(rng.integers(0, w - 30)) + 0.5 * (k % 2), float(rng.integers(0, h - 30))
        b = {"class": CLASSES[k % len(CLASSES)], "confidence": 0.5, "xmin": x, "ymin": y, "xmax": x + float(rng.integers(8, 30)), "ymax": y + float(rng.integers(8, 30)) + 0.25}
        if k % 5 != 3:
            b["persistent_uid"] = f"u{k % 7}"                           # some boxes share a uid, some have none
        bb.append(b)
    return bb


def _assert_same_result(g, w, what=""):
    assert np.array_equal(g["emptied_mask"].cpu().numpy(), w["emptied_mask"]) and np.array_equal(g["enhanced"].cpu().numpy(), w["enhanced"]), what
    assert g["resized_bboxes"] == w["resized_bboxes"], what
    assert [(d["id"], d["area"], d["rectangle"]) for d in g["contours"]] == [(d["id"], d["area"], d["rectangle"]) for d in w["contours"]], what
    assert [n["id"] for n in g["nodes"]] == [n["id"] for n in w["nodes"]], what
    for a, b in zip(g["nodes"], w["nodes"]):
        assert a["components"] == b["components"], (what, a["id"])     # the same dicts in the same order
        assert a["contour"].dtype == np.int32 and np.array_equal(a["contour"], b["contour"]), (what, a["id"])
    assert [(int(x), int(y)) for x, y in g["connection_points"]] == [(int(x), int(y)) for x, y in w["connection_points"]], what


def test_node_connections_batch_equals_the_reference_composition():
    rng = np.random.default_rng(5)
    shapes = [(150, 200), (131, 97), (96, 260), (160, 160)]
    masks = [_wire(h, w, 40 + i) for i, (h, w) in enumerate(shapes)]
    boxes = [_boxes(rng, h, w, 9 + 4 * i) for i, (h, w) in enumerate(shapes)]
    boxes[1] = [b for b in boxes[1] if b["class"] in ("text", "junction")]                      # a plane whose loop visits no box
    got = wires.node_connections([_dev(m) for m in masks], boxes, new_height=128)
    some = 0
    for i, (m, bb) in enumerate(zip(masks, boxes)):
        want = R.node_connections(m, bb, new_height=128)
        _assert_same_result(got[i], want, i)
        some += len(want["nodes"])
    assert some >= 3 and got[1]["nodes"] == [] and got[1]["connection_points"] == []
    # one image at the default height of 600
    g = wires.node_connections([_dev(masks[0])], [boxes[0]])[0]
    want = R.node_connections(masks[0], boxes[0])
    assert g["enhanced"].shape[0] == 600 and len(want["nodes"]) >= 1
    _assert_same_result(g, want, "600")
    assert wires.node_connections([], []) == []


def test_get_node_connections_returns_the_reference_six_tuple():
    rng = np.random.default_rng(6)
    m = _wire(75, 100, 50)
    bb = _boxes(rng, 75, 100, 8)
    img = np.zeros((75, 100, 3), np.uint8)
    got = wires.get_node_connections(img, m.copy(), bb)
    want = R.get_node_connections(img, m.copy(), bb)
    assert len(got) == 6 and len(want[0]) >= 1
    assert [n["id"] for n in got[0]] == [n["id"] for n in want[0]]
    assert all(a["components"] == b["components"] and np.array_equal(a["contour"], b["contour"]) for a, b in zip(got[0], want[0]))
    for k in range(1, 6):
        assert isinstance(got[k], np.ndarray) and got[k].dtype == np.uint8 and got[k].shape == want[k].shape, k
    assert got[1].shape == (75, 100) and got[2].shape == (600, 800) and got[3].shape == (600, 800, 3)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and not any(got[k].any() for k in (3, 4, 5))
    # a device mask: the two planes stay on the device
    dev = wires.get_node_connections(None, _dev(m), bb)
    assert dev[1].is_cuda and dev[2].is_cuda and np.array_equal(dev[2].cpu().numpy(), want[2]) and [n["id"] for n in dev[0]] == [n["id"] for n in want[0]]
    # no valid node: boxes the loop does not visit
    none = wires.get_node_connections(img, m.copy(), [b for b in bb if b["class"] in ("text", "junction", "crossover")])
    assert none[0] == [] and none[1].shape == (75, 100) and none[2].shape == (600, 800) and all(none[k].shape == (600, 800, 3) for k in (3, 4, 5))
    # no mask
    for image, hw in ((img, (75, 100)), (None, (100, 100))):
        out = wires.get_node_connections(image, None, bb)
        assert out[0] == [] and all(o.shape == hw + (3,) and o.dtype == np.uint8 and not o.any() for o in out[1:])


def test_pipeline_connections_equal_node_connections_and_nodes_true_keeps_its_keys(tmp_path):
    from circuitvision_amd.pipeline import CircuitPipeline
    from test_pipeline_gpu import _mini_setup
    images, det, yo, seg, tr, so, R_ = _mini_setup(tmp_path, n_images=3)
    base = CircuitPipeline(det, seg, tr, seg_batch=2).run_batch(images, "learned")
    on = CircuitPipeline(det, seg, tr, seg_batch=2, nodes=True)
    full = CircuitPipeline(det, seg, tr, seg_batch=2, nodes="connections")
    b, c = on.run_batch(images, "learned"), full.run_batch(images, "learned")
    want = wires.node_connections([r["mask"] for _, r in c], [r["bboxes"] for _, r in c])
    for (_, ra), (_, rb), (_, rc), w in zip(base, b, c, want):
        assert set(rb) == set(ra) | {"emptied_mask", "resized_bboxes", "enhanced", "contours"}
        assert set(rc) == set(rb) | {"nodes", "connection_points"}
        assert torch.equal(rc["mask"], ra["mask"]) and rc["bboxes"] == ra["bboxes"]
        assert [n["id"] for n in rc["nodes"]] == [n["id"] for n in w["nodes"]] and rc["connection_points"] == w["connection_points"]
        assert all(x["components"] == y["components"] and np.array_equal(x["contour"], y["contour"]) for x, y in zip(rc["nodes"], w["nodes"]))
        assert torch.equal(rc["enhanced"], w["enhanced"]) and rc["resized_bboxes"] == w["resized_bboxes"]
    assert any("connections" in k for k in full.timings if k.startswith("nodes")) and not any("connections" in k for k in on.timings)
    with pytest.raises(ValueError):
        full.run_batch(images, "boxes")
    with pytest.raises(ValueError):
        CircuitPipeline(det, seg, tr, nodes="netlist")
