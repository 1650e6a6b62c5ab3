"""Node-analysis front end on the GPU (wire_ops.hip via circuitvision_amd.wires) against tests/wire_ref.py, bit for bit."""
import numpy as np
import pytest
import torch

import wire_ref as W
from circuitvision_amd import wires
from synth import circuit_image

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _packed(planes):
    buf = torch.cat([_dev(p).reshape(-1) for p in planes])
    return buf, [p.shape for p in planes]


def _unpack(buf, shapes):
    out, o = [], 0
    flat = buf.cpu().numpy()
    for h, w in shapes:
        out.append(flat[o:o + h * w].reshape(h, w))
        o += h * w
    return out


def _wire(h, w, seed):
    return W.wire_mask(circuit_image(h, w, seed=seed))


def _ref_contours(plane):
    """(points, 2 x signed area, rect) per external contour of the plane as get_contours sees it (inversion included)."""
    p = 255 - plane if W.plane_sum_inverts(plane) else plane
    return [(pts, W.shoelace2(pts), W.bounding_rect(pts)) for pts in W.find_external_contours(p != 0)]


def _assert_same_contours(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, ((gp, ga, gr), (wp, wa, wr)) in enumerate(zip(got, want)):
        assert [tuple(v) for v in gp.tolist()] == wp, (what, k)
        assert ga == wa and tuple(gr) == wr, (what, k, ga, wa, gr, wr)


# ---- preparation ----------------------------------------------------------------------------------------------------------------
def test_prepare_matches_the_reference_on_mixed_sizes_and_awkward_boxes():
    rng = np.random.default_rng(0)
    shapes = [(300, 420), (257, 311), (600, 800), (41, 13), (599, 1001)]
    masks = [np.where(rng.random(s) < 0.2, 255, 0).astype(np.uint8) for s in shapes]
    masks[1] = _wire(257, 311, 3)
    boxes = []
    for h, w in shapes:
        bb = [{"class": "resistor", "xmin": -15.5, "ymin": -3, "xmax": 20.9, "ymax": 30.2},          # negative
              {"class": "capacitor", "xmin": w - 10, "ymin": h - 7, "xmax": w + 50, "ymax": h + 99},  # past the edge
              {"class": "inductor", "xmin": 30, "ymin": 30, "xmax": 30, "ymax": 60},                 # empty
              {"class": "junction", "xmin": 0, "ymin": 0, "xmax": w, "ymax": h},                     # preserved
              {"class": "vss", "xmin": 5, "ymin": 5, "xmax": 50, "ymax": 50},                        # preserved
              {"class": "diode", "xmin": w // 3, "ymin": h // 4, "xmax": w // 2 + 0.7, "ymax": h // 2 + 0.2}]
        boxes.append(bb)
    boxes[3] = []                                                                                  # a plane with no box
    src, _ = _packed(masks)
    emptied, resized, new_shapes = wires.prepare_packed(src, shapes, boxes)
    got_e, got_r = _unpack(emptied, shapes), _unpack(resized, new_shapes)
    for i, (m, bb) in enumerate(zip(masks, boxes)):
        e = W.empty_boxes(m, bb)
        r, _ = W.resize_keep_aspect(e, bb)
        assert np.array_equal(got_e[i], e), i
        assert got_r[i].shape == r.shape and np.array_equal(got_r[i], r), i


# ---- enhance_lines ----------------------------------------------------------------------------------------------------------------
def test_enhance_matches_bit_for_bit_with_exact_sums():
    rng = np.random.default_rng(1)
    planes = [rng.integers(0, 256, (h, w), dtype=np.uint8) for h in range(1, 8) for w in range(1, 8)]
    planes += [rng.integers(0, 256, (33, 65), dtype=np.uint8), rng.integers(0, 256, (97, 130), dtype=np.uint8)]
    planes += [np.where(rng.random((h, w)) < 0.3, 255, 0).astype(np.uint8) for h, w in ((5, 3), (64, 64), (31, 129), (600, 803))]
    planes += [_wire(600, 812, 4)]
    src, shapes = _packed(planes)
    out, sums = wires.enhance_packed(src, shapes)
    got = _unpack(out, shapes)
    sums = sums.cpu().numpy()
    for i, p in enumerate(planes):
        want = W.enhance_lines(p)
        assert np.array_equal(got[i], want), (i, p.shape)
        assert int(sums[i]) == int(want.astype(np.int64).sum()), i


def test_enhance_lines_wrapper_numpy_and_tensor():
    p = _wire(150, 221, 9)
    want = W.enhance_lines(p)
    a = wires.enhance_lines(p)
    b = wires.enhance_lines(_dev(p))
    assert isinstance(a, np.ndarray) and np.array_equal(a, want)
    assert torch.is_tensor(b) and b.is_cuda and np.array_equal(b.cpu().numpy(), want)


# ---- external contours ------------------------------------------------------------------------------------------------------------
def _rings(h=120, w=160):
    m = np.zeros((h, w), np.uint8)
    for k in range(0, 50, 6):                                       # nested square rings, a dot in the middle
        m[10 + k, 10 + k:110 - k] = 255
        m[109 - k, 10 + k:110 - k] = 255
        m[10 + k:110 - k, 10 + k] = 255
        m[10 + k:110 - k, 109 - k] = 255
    m[59, 59] = 255
    m[5:20, 130:150] = 255
    m[50:70, 125:155] = 255
    m[55:65, 130:150] = 0                                           # a ring with a hole next to the nest
    m[60, 140] = 255
    return m


def _contour_planes():
    rng = np.random.default_rng(2)
    planes = [W.enhance_lines(_wire(600, 800, s)) for s in (11, 12)]
    planes += [np.where(rng.random((600, 800)) < 0.35, 255, 0).astype(np.uint8)]          # thousands of components
    planes += [np.zeros((40, 50), np.uint8), np.full((37, 41), 255, np.uint8), _rings()]
    planes += [np.where(rng.random((7, 5)) < 0.5, 255, 0).astype(np.uint8), np.full((1, 1), 255, np.uint8)]
    return planes


def test_contours_match_points_order_area_rectangles_and_counts():
    planes = _contour_planes()
    src, shapes = _packed(planes)
    _, sums = wires.enhance_packed(src, shapes)                     # any plane: only the sums are used here
    sums = torch.tensor([int(p.astype(np.int64).sum()) for p in planes], dtype=torch.int64, device="cuda")
    pc = wires.contours_packed(src, shapes, sums, binarize=True)
    assert pc.longest_border > 0
    for i, p in enumerate(planes):
        want = _ref_contours(p)
        _assert_same_contours(pc.plane(i), want, i)
        assert int(pc.counts[i]) == len(want)
    assert len(_ref_contours(planes[2])) > 1000
    assert pc.counts[3] == 0 and pc.counts[4] == 0                  # all zero; all 255 inverts to all zero
    # binarize: 255 -> 1 in the planes that did not invert, the inverted ones untouched
    after = _unpack(src, shapes)
    for i, p in enumerate(planes):
        want = p.copy()
        if not W.plane_sum_inverts(p):
            want[want == 255] = 1
        assert np.array_equal(after[i], want), i


def test_contours_past_the_first_guess_capacity_are_complete():
    rng = np.random.default_rng(3)
    planes = [np.where(rng.random((300, 400)) < 0.3, 255, 0).astype(np.uint8) for _ in range(2)]
    src, shapes = _packed(planes)
    pc = wires.contours_packed(src, shapes, None, binarize=False, cap_contours=16, cap_points=64)
    for i, p in enumerate(planes):
        _assert_same_contours(pc.plane(i), _ref_contours(p), i)
    assert int(pc.counts[:2].sum()) > 16


def test_get_contours_wrapper_equals_the_reference_dicts():
    for p in (W.enhance_lines(_wire(600, 790, 21)), 255 - W.enhance_lines(_wire(300, 450, 22))):
        a, b = p.copy(), p.copy()
        want, _ = W.get_contours(a)
        got, canvas = wires.get_contours(b)
        assert np.array_equal(a, b)                                  # the same in-place 255 -> 1 (or none, when inverted)
        assert canvas.shape == p.shape + (3,) and canvas.dtype == np.uint8 and not canvas.any()
        assert len(got) == len(want) > 0
        for g, w in zip(got, want):
            assert g["id"] == w["id"] and g["area"] == w["area"] and g["rectangle"] == w["rectangle"]
            assert g["contour"].dtype == np.int32 and np.array_equal(g["contour"], w["contour"])
        t = torch.from_numpy(p.copy()).cuda()
        got_t, _ = wires.get_contours(t)
        assert np.array_equal(t.cpu().numpy(), a) and [g["rectangle"] for g in got_t] == [w["rectangle"] for w in want]


def test_node_contours_batch_equals_the_reference_composition():
    shapes = [(300, 420), (401, 333), (212, 640)]
    masks = [_wire(h, w, 30 + i) for i, (h, w) in enumerate(shapes)]
    boxes = [[{"class": "resistor", "xmin": 40, "ymin": 50, "xmax": 90.6, "ymax": 120},
              {"class": "junction", "xmin": 100, "ymin": 100, "xmax": 150, "ymax": 150}] for _ in shapes]
    got = wires.node_contours([_dev(m) for m in masks], boxes)
    for i, (m, bb) in enumerate(zip(masks, boxes)):
        e, rb, enh, cs = W.node_contours(m, bb)
        g = got[i]
        assert np.array_equal(g["emptied_mask"].cpu().numpy(), e) and g["resized_bboxes"] == rb
        assert np.array_equal(g["enhanced"].cpu().numpy(), enh)
        assert len(g["contours"]) == len(cs)
        for a, b in zip(g["contours"], cs):
            assert a["id"] == b["id"] and a["area"] == b["area"] and a["rectangle"] == b["rectangle"]
            assert np.array_equal(a["contour"], b["contour"])


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------
def test_pipeline_nodes_equal_the_reference_composition(tmp_path):
    from circuitvision_amd.pipeline import CircuitPipeline
    from test_pipeline_gpu import _mini_setup
    images, det, yo, seg, tr, so, R = _mini_setup(tmp_path, n_images=3)
    for crop in (False, True):
        base = CircuitPipeline(det, seg, tr, seg_batch=2, crop=crop)
        off = CircuitPipeline(det, seg, tr, seg_batch=2, crop=crop, nodes=False)
        on = CircuitPipeline(det, seg, tr, seg_batch=2, crop=crop, nodes=True)
        a, b, c = base.run_batch(images, "learned"), off.run_batch(images, "learned"), on.run_batch(images, "learned")
        for (i, ra), (j, rb), (k, rc) in zip(a, b, c):
            assert i == j == k and set(ra) == set(rb) and ra["bboxes"] == rb["bboxes"] and torch.equal(ra["mask"], rb["mask"])
            assert "contours" not in rb
            assert rc["bboxes"] == ra["bboxes"] and torch.equal(rc["mask"], ra["mask"])
            e, rbb, enh, cs = W.node_contours(rc["mask"].cpu().numpy(), rc["bboxes"])
            assert np.array_equal(rc["emptied_mask"].cpu().numpy(), e) and rc["resized_bboxes"] == rbb
            assert np.array_equal(rc["enhanced"].cpu().numpy(), enh)
            assert [(d["id"], d["area"], d["rectangle"]) for d in rc["contours"]] == [(d["id"], d["area"], d["rectangle"]) for d in cs]
            assert all(np.array_equal(x["contour"], y["contour"]) for x, y in zip(rc["contours"], cs))
        assert any(key.startswith("nodes") for key in on.timings) and not any(key.startswith("nodes") for key in off.timings)
    with pytest.raises(ValueError):
        CircuitPipeline(det, seg, tr, nodes=True).run_batch(images, "boxes")
