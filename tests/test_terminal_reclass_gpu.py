"""Terminal reclassification on the GPU (cvmi_segment_circuit, cvmi_contour_hits via circuitvision_amd.wires) against tests/segment_ref.py,
bit for bit: the fused grey / 31 x 31 mean / threshold / emptying kernel on packed planes of every size class, windows of a larger image,
rectangles, the hit table without a broad phase, the batched and the reference-shaped wrappers, and the pipeline switch."""
import json
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

import node_ref as R
import segment_ref as S
import wire_ref as W
from circuitvision_amd import wires
from synth import circuit_image

pytestmark = pytest.mark.gpu

TW, TH = 128, 64                                                       # STW x STH of wire_ops.hip: the segment kernel's output tile
PLANE_MAX = 32                                                         # planes whose geometry travels in one launch
RECT_TILE = 256                                                        # SRECT_TILE: rectangles in LDS at a time
NAMES = {0: "resistor", 1: "terminal", 2: "voltage.dc", 3: "junction", 4: "text"}
HERE = os.path.dirname(os.path.abspath(__file__))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rgb(g):
    """A grey plane as an RGB image: the three weights sum to 2^15, so grey((v, v, v)) == v."""
    return np.repeat(g[..., None], 3, axis=2)


def _segment(images, rects=None, red=0):
    """cvmi_segment_circuit on contiguous images packed back to back: -> (u8 masks, python-int sums, packed device masks, device sums)."""
    flat = torch.cat([_dev(im).reshape(-1) for im in images])
    planes, off = [], 0
    for im in images:
        h, w = im.shape[:2]
        planes.append((off, 3 * w, h, w))
        off += 3 * h * w
    masks, sums = wires.segment_packed(flat, planes, rects if rects is not None else [[] for _ in images], red)
    assert masks.dtype == torch.uint8 and sums.dtype == torch.int64 and masks.numel() == sum(im.shape[0] * im.shape[1] for im in images)
    host, out, o = masks.cpu().numpy(), [], 0
    for im in images:
        h, w = im.shape[:2]
        out.append(host[o:o + h * w].reshape(h, w))
        o += h * w
    return out, [int(v) for v in sums.cpu().tolist()], masks, sums


def _noise_planes():
    rng = np.random.default_rng(0)
    noise = rng.integers(0, 256, size=(97, 131), dtype=np.uint8)
    mostly_zero = np.where(rng.random((97, 131)) > 0.4, 0, 255).astype(np.uint8)       # 60 % zeros: the threshold's output is mostly white
    return noise, mostly_zero


@pytest.fixture(scope="module")
def batch():
    """One packed batch of every size class, its images and the restatement's masks for both channel orders (computed once)."""
    rng = np.random.default_rng(11)
    sizes = [(1, 1), (1, 40), (40, 1), (15, 15), (31, 33)] + [(h, w) for h in (TH - 1, TH, TH + 1) for w in (TW - 1, TW, TW + 1)]
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]    # channels differ
    noise, mostly_zero = _noise_planes()
    images += [_rgb(noise), _rgb(mostly_zero)] + [circuit_image(120, 200, seed=s) for s in (1, 2, 3)]
    return images, {red: [S.segment_circuit(im, red) for im in images] for red in (0, 2)}


# ---- cvmi_segment_circuit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("red", [0, 2])
def test_segment_circuit_on_one_packed_batch_of_every_size_class(batch, red):
    images, want = batch
    got, sums, _, _ = _segment(images, red=red)
    for k, (g, w) in enumerate(zip(got, want[red])):
        assert np.array_equal(g, w), (k, images[k].shape, int((g != w).sum()))
        assert sums[k] == int(w.astype(np.int64).sum()), k
    assert any(not np.array_equal(a, b) for a, b in zip(want[0], want[2]))              # the channel order matters on these images
    assert all(set(np.unique(g)) <= {0, 255} for g in got)


def test_plane_sums_trigger_the_inversion_downstream_and_the_contours_are_the_restatement(batch):
    images, want = batch
    pick = [len(images) - 5, len(images) - 4, len(images) - 3, len(images) - 2, len(images) - 1]      # noise, 60 % zeros, three circuit images
    sub = [images[k] for k in pick]
    _, sums, masks, dsums = _segment(sub)
    shapes = [im.shape[:2] for im in sub]
    inverts = [s > 127 * h * w for s, (h, w) in zip(sums, shapes)]
    assert inverts[1] and not all(inverts)
    pc = wires.contours_packed(masks, shapes, dsums, binarize=True)
    for j, k in enumerate(pick):
        ref, _ = W.get_contours(want[0][k].copy(), S.AREA)
        got = wires.contour_dicts(pc.plane(j), *shapes[j], S.AREA)
        assert [c["rectangle"] for c in got] == [tuple(c["rectangle"]) for c in ref], k
        assert all(np.array_equal(a["contour"], b["contour"]) for a, b in zip(got, ref)), k
    n_circuit = [len(wires.contour_dicts(pc.plane(j), *shapes[j], S.AREA)) for j in (2, 3, 4)]
    assert all(n >= 2 for n in n_circuit), n_circuit


def test_one_more_plane_than_a_launch_carries():
    rng = np.random.default_rng(2)
    images = [rng.integers(0, 256, size=(int(rng.integers(1, 9)), int(rng.integers(1, 9)), 3), dtype=np.uint8) for _ in range(PLANE_MAX + 1)]
    images[-1] = rng.integers(0, 256, size=(40, 50, 3), dtype=np.uint8)                  # the plane of the second launch is not trivial
    rects = [[] for _ in images]
    rects[-1] = [[3, 4, 20, 30]]
    got, sums, _, _ = _segment(images, rects)
    for k, im in enumerate(images):
        w = S.segment_circuit(im, 0)
        if k == PLANE_MAX:
            w[4:30, 3:20] = 0
        assert np.array_equal(got[k], w) and sums[k] == int(w.astype(np.int64).sum()), k
    assert sums[-1] > 0


def test_a_window_of_a_larger_image_equals_its_cropped_copy():
    rng = np.random.default_rng(3)
    H, Wd = 150, 211                                                   # pitch 633 bytes: no multiple of 4
    windows = [(17, 9, 17 + TW + 5, 9 + TH + 3), (0, 0, 40, 33), (Wd - 37, H - 20, Wd, H), (100, 70, 101, 71)]      # (x0, y0, x1, y1)
    big = np.zeros((2, H, Wd, 3), np.uint8)                             # outside the windows: 0, which would pull every border mean down
    for b in range(2):
        for x0, y0, x1, y1 in windows:
            big[b, y0:y1, x0:x1] = rng.integers(150, 256, size=(y1 - y0, x1 - x0, 3), dtype=np.uint8)
    crops = [np.ascontiguousarray(big[b, y0:y1, x0:x1]) for b in range(2) for x0, y0, x1, y1 in windows]
    planes = [(((b * H + y0) * Wd + x0) * 3, 3 * Wd, y1 - y0, x1 - x0) for b in range(2) for x0, y0, x1, y1 in windows]
    masks, sums = wires.segment_packed(_dev(big).view(-1), planes, [[] for _ in planes], 2)
    host, o = masks.cpu().numpy(), 0
    want_crops, _, _, _ = _segment(crops, red=2)
    for k, c in enumerate(crops):
        h, w = c.shape[:2]
        ref = S.segment_circuit(c, 2)
        got = host[o:o + h * w].reshape(h, w)
        o += h * w
        assert np.array_equal(got, ref) and np.array_equal(want_crops[k], ref), k
        assert int(sums[k]) == int(ref.astype(np.int64).sum())
    x0, y0, x1, y1 = windows[0]
    assert not np.array_equal(S.segment_circuit(big[0], 2)[y0:y1, x0:x1], S.segment_circuit(crops[0], 2))         # the image's border is not the window's
    with pytest.raises(wires._lib.CvmiError):                                                                        # a window that leaves the buffer
        wires.segment_packed(_dev(big).view(-1), [(((1 * H + H - 5) * Wd) * 3, 3 * Wd, 6, Wd)], [[]], 0)


def test_rectangles_partly_outside_empty_negative_stop_more_than_one_tile_and_exact_sums():
    rng = np.random.default_rng(4)
    h, w = 100, 150
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(2)]
    few = [{"class": "resistor", "xmin": -20, "ymin": 70, "xmax": 30, "ymax": 140}, {"class": "text", "xmin": 60, "ymin": 10, "xmax": 60, "ymax": 50},
           {"class": "terminal", "xmin": 100, "ymin": 0, "xmax": -10, "ymax": h}, {"class": "gnd", "xmin": 40, "ymin": 60, "xmax": 90, "ymax": -30},
           {"class": "junction", "xmin": 0, "ymin": 0, "xmax": w, "ymax": h}, {"class": "diode", "xmin": 149, "ymin": 99, "xmax": 400, "ymax": 400}]
    many = []
    for _ in range(2 * RECT_TILE + 19):
        x, y = int(rng.integers(0, w - 4)), int(rng.integers(0, h - 4))
        many.append({"class": "resistor", "xmin": x, "ymin": y, "xmax": x + int(rng.integers(1, 5)), "ymax": y + int(rng.integers(1, 5))})
    boxes = [few, many]
    rects = [wires.emptying_rects(bb, h, w) for bb in boxes]
    assert len(rects[0]) == 4 and len(rects[1]) == len(many)
    got, sums, _, _ = _segment(images, rects)
    for k in range(2):
        want = S.empty_boxes(S.segment_circuit(images[k], 0), boxes[k])
        assert np.array_equal(got[k], want) and sums[k] == int(want.astype(np.int64).sum()), k
    assert not np.array_equal(got[1], S.empty_boxes(S.segment_circuit(images[1], 0), many[:RECT_TILE]))              # the later tiles count
    assert not got[0][:, 100:140].any() and got[0][:60, 40:90].any()


# ---- cvmi_contour_hits ---------------------------------------------------------------------------------------------------------------
def _first_no_broad_phase(pts, box, t):
    for i, p in enumerate(pts):
        if R.is_point_near_bbox(p, box, t):
            return i
    return -1


def _box(r):
    return {"xmin": r[0], "ymin": r[1], "xmax": r[2], "ymax": r[3]}


def test_hits_table_has_no_broad_phase():
    rng = np.random.default_rng(5)
    wires_mask = np.zeros((200, 240), np.uint8)
    for x0, y0, x1, y1 in ([100, 50, 200, 54], [140, 100, 215, 104], [180, 150, 230, 154]):
        wires_mask[y0:y1, x0:x1] = 255
    planes = [wires_mask, W.wire_mask(circuit_image(120, 160, seed=11)), np.zeros((30, 40), np.uint8),
              np.where(rng.random((97, 131)) < 0.3, 255, 0).astype(np.uint8)]
    rows = [[[55, 130, 98, 140, 10], [9, 13, 37, 81, 10], [150, 40, 160, 60, 10]]]     # the first: overlaps no wire's rectangle, two edge lines pass wire ends
    for p in planes[1:]:
        rr = []
        for _ in range(6):
            x, y = int(rng.integers(-10, p.shape[1])), int(rng.integers(-10, p.shape[0]))
            rr.append([x, y, x + int(rng.integers(0, 40)), y + int(rng.integers(0, 40)), 10])
        rows.append(rr)
    rows[3] = []
    shapes = [p.shape for p in planes]
    buf = torch.cat([_dev(p).reshape(-1) for p in planes])
    pc, info, points = wires.contours_packed(buf, shapes, None, binarize=False, keep_device=True)
    box_start = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    per_plane = np.asarray(pc.counts[:len(planes)], dtype=np.int64)
    pair_start = np.concatenate(([0], np.cumsum(np.repeat(np.diff(box_start), per_plane))))
    flat = [r for rr in rows for r in rr]
    hits = wires.hits_packed(info, points, flat, box_start, pair_start)
    assert hits.dtype == torch.int32 and hits.numel() == int(pair_start[-1])
    hits = hits.cpu().numpy()
    broad, _ = wires.connect_packed(info, points, flat, box_start, pair_start)
    broad = broad.cpu().numpy()
    c, differ = 0, 0
    for n, rr in enumerate(rows):
        for pts, _a2, rect in pc.plane(n):
            pts = [tuple(v) for v in pts.tolist()]
            got = hits[pair_start[c]:pair_start[c + 1]].tolist()
            assert got == [_first_no_broad_phase(pts, _box(r), r[4]) for r in rr], (n, c)
            assert broad[pair_start[c]:pair_start[c + 1]].tolist() == [R.first_near(pts, tuple(rect), _box(r), r[4]) for r in rr], (n, c)
            differ += sum(a != b for a, b in zip(got, broad[pair_start[c]:pair_start[c + 1]].tolist()))
            c += 1
    assert c == len(pair_start) - 1 and differ >= 2
    # the edge-line box on the three wires: found on wires 0 and 2 here, on none with the broad phase
    first3 = [hits[pair_start[k]] for k in range(3)]
    assert sorted(int(f >= 0) for f in first3) == [0, 1, 1] and all(broad[pair_start[k]] == -1 for k in range(3))
    assert len(pc.plane(0)) == 3 and len(pc.plane(2)) == 0 and len(pc.plane(3)) > 3


# ---- the wrappers --------------------------------------------------------------------------------------------------------------------
def _term_boxes(rng, h, w, n):
    classes = ["terminal", "resistor", "terminal", "junction", "text", "terminal", "voltage.dc"]
    bb = []
    for k in range(n):
        x, y = int(rng.integers(-5, w - 10)), int(rng.integers(-5, h - 10))
        bb.append({"class": classes[k % len(classes)], "_yolo_class_id_temp": 1, "confidence": 0.5, "xmin": x, "ymin": y, "xmax": x + int(rng.integers(4, 40)),
                   "ymax": y + int(rng.integers(4, 40)), "persistent_uid": f"u{k}"})
    return bb


def test_reclassify_terminals_on_a_batch_of_different_sizes_equals_the_restatement_per_image():
    rng = np.random.default_rng(6)
    images = [circuit_image(120, 200, seed=1), circuit_image(90, 141, seed=2), S.segments_image(200, 240, 1, [[100, 50, 200, 54], [140, 100, 215, 104], [180, 150, 230, 154]]),
              circuit_image(70, 66, seed=3), circuit_image(130, 100, seed=4)]
    boxes = [_term_boxes(rng, *im.shape[:2], 5 + 2 * k) for k, im in enumerate(images)]
    boxes[2] = [{"class": "terminal", "xmin": 55.0, "ymin": 130.0, "xmax": 98.0, "ymax": 140.0}, {"class": "terminal", "xmin": 9, "ymin": 13, "xmax": 37, "ymax": 81}]
    boxes[3] = [b for b in boxes[3] if b["class"] != "terminal"]                         # an image without terminals is left alone
    for red in (0, 2):
        want_boxes, want_counts = deepcopy(boxes), []
        for im, bb in zip(images, want_boxes):
            want_counts.append(S.reclassify(im, bb, NAMES, red)[0])
        got_boxes = deepcopy(boxes)
        inputs = [_dev(im) if k % 2 else im for k, im in enumerate(images)]               # device tensors and numpy arrays
        got = wires.reclassify_terminals(inputs, got_boxes, NAMES, red_channel=red)
        assert got == want_counts and got_boxes == want_boxes, red
        assert got[3] == {} and got_boxes[3] == boxes[3]
        assert any(v >= 2 for c in got for v in c.values()) and any(v < 2 for c in got for v in c.values())
        changed = [b for bb in got_boxes for b in bb if b.get("was_reclassified_from_terminal")]
        assert changed and all(b["class"] == "voltage.dc" and b["_yolo_class_id_temp"] == 2 and b["original_yolo_class_if_reclassified"] == "terminal" for b in changed)
    assert wires.reclassify_terminals([], [], NAMES) == []
    # windows of one device block equal the cropped copies
    block = np.stack([circuit_image(120, 200, seed=5), circuit_image(120, 200, seed=6)])
    wins = [(20, 10, 171, 101), None]
    crops = [np.ascontiguousarray(block[0][10:101, 20:171]), block[1]]
    bb = [_term_boxes(rng, 91, 151, 6), _term_boxes(rng, 120, 200, 6)]
    a, b = deepcopy(bb), deepcopy(bb)
    assert wires.reclassify_terminals(_dev(block), a, NAMES, windows=wins) == [S.reclassify(c, x, NAMES, 0)[0] for c, x in zip(crops, b)] and a == b


def test_non_integral_terminal_coordinates_raise():
    img = circuit_image(60, 80, seed=1)
    with pytest.raises(ValueError):
        wires.reclassify_terminals([img], [[{"class": "terminal", "xmin": 5.5, "ymin": 5, "xmax": 20, "ymax": 20}]], NAMES)
    bb = [[{"class": "resistor", "xmin": 5.5, "ymin": 5.2, "xmax": 20.9, "ymax": 20.1}, {"class": "terminal", "xmin": 30.0, "ymin": 30.0, "xmax": 50.0, "ymax": 50.0}]]
    want = deepcopy(bb)
    assert wires.reclassify_terminals([img], bb, NAMES) == [S.reclassify(img, want[0], NAMES, 0)[0]] and bb == want       # int() of the emptied boxes, as the reference


def test_reference_shaped_methods_equal_the_fixture():
    with open(os.path.join(HERE, "golden", "terminal_reclass.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 9
    for c in cases:
        img = S.golden_image(c["image"])
        bb = [dict(b) for b in c["bboxes"]]
        assert wires.reclassify_terminals_based_on_connectivity(img, bb, {int(k): v for k, v in c["names"].items()}) is None
        assert bb == c["expect"]["bboxes"], c["name"]
        m = wires.segment_circuit(img)
        assert isinstance(m, np.ndarray) and m.dtype == np.uint8 and S.mask_summary(m) == c["expect"]["segment_circuit"], c["name"]
    img = S.golden_image(cases[0]["image"])
    t = wires.segment_circuit(_dev(img))
    assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), S.segment_circuit(img, 0))
    with pytest.raises(ValueError):
        wires.segment_circuit(img[..., 0])


# ---- the pipeline switch --------------------------------------------------------------------------------------------------------------
def test_pipeline_reclassify_switch(tmp_path):
    from circuitvision_amd.crop import crop_image_and_adjust_bboxes
    from circuitvision_amd.pipeline import CircuitPipeline
    from test_pipeline_gpu import _mini_setup
    images, det, yo, seg, tr, so, R_ = _mini_setup(tmp_path, n_images=3)
    probe = CircuitPipeline(det, seg, tr, seg_batch=2).run_batch(images, "learned")
    ids = [b["_yolo_class_id_temp"] for _, r in probe for b in r["bboxes"]]
    by_count = sorted(set(ids), key=lambda i: (-ids.count(i), i))
    other = by_count[1] if len(by_count) > 1 else (by_count[0] + 1) % len(det.names)
    det.names[by_count[0]], det.names[other] = "terminal", "voltage.dc"                   # the most frequent class: the step has work
    base = CircuitPipeline(det, seg, tr, seg_batch=2, reclassify=False).run_batch(images, "learned")
    for (_, ra), (_, rp) in zip(base, probe):
        assert set(ra) == set(rp) == {"image", "bboxes", "mask", "extent", "iou"} and torch.equal(ra["mask"], rp["mask"]) and ra["extent"] == rp["extent"]
        assert [(b["xmin"], b["ymin"], b["xmax"], b["ymax"], b["_yolo_class_id_temp"]) for b in ra["bboxes"]] == \
            [(b["xmin"], b["ymin"], b["xmax"], b["ymax"], b["_yolo_class_id_temp"]) for b in rp["bboxes"]]
    assert sum(b["class"] == "terminal" for _, r in base for b in r["bboxes"]) >= 1
    on = CircuitPipeline(det, seg, tr, seg_batch=2, reclassify=True)
    got = on.run_batch(images, "learned")
    want_boxes = [deepcopy(r["bboxes"]) for _, r in base]
    want_counts = wires.reclassify_terminals([r["image"] for _, r in base], want_boxes, det.names, red_channel=0)
    host_boxes = [deepcopy(r["bboxes"]) for _, r in base]
    for k, ((_, rg), (_, rb)) in enumerate(zip(got, base)):
        assert set(rg) == set(rb) | {"terminal_connections"} and torch.equal(rg["mask"], rb["mask"])
        assert rg["bboxes"] == want_boxes[k] and rg["terminal_connections"] == want_counts[k], k
        assert S.reclassify(images[k], host_boxes[k], det.names, 0)[0] == want_counts[k] and host_boxes[k] == want_boxes[k], k
    print("terminal connections per image:", want_counts)
    for bb, cnt in zip(want_boxes, want_counts):                                           # the rule, whatever the counts on these images are
        assert all((cnt[k] >= 2) == (b["class"] == "voltage.dc" and b.get("was_reclassified_from_terminal") is True) for k, b in enumerate(bb) if k in cnt)
        assert all(b["class"] != "terminal" or k in cnt for k, b in enumerate(bb))
    assert any(k.startswith("reclassify") for k in on.timings)
    # node analysis reads the rewritten boxes
    full = CircuitPipeline(det, seg, tr, seg_batch=2, nodes="connections", reclassify=True).run_batch(images, "learned")
    want_nodes = wires.node_connections([r["mask"] for _, r in full], want_boxes)
    for k, ((_, rf), w) in enumerate(zip(full, want_nodes)):
        assert rf["bboxes"] == want_boxes[k] and rf["resized_bboxes"] == w["resized_bboxes"], k
        assert [n["id"] for n in rf["nodes"]] == [n["id"] for n in w["nodes"]] and rf["connection_points"] == w["connection_points"], k
        assert all(x["components"] == y["components"] and np.array_equal(x["contour"], y["contour"]) for x, y in zip(rf["nodes"], w["nodes"])), k
    # box prompts: the step runs there too
    boxes_mode = CircuitPipeline(det, seg, tr, seg_batch=2, max_prompts=6, reclassify=True).run_batch(images, "boxes")
    assert all("terminal_connections" in r and "masks" in r for _, r in boxes_mode)
    # the cropped chain reads the windows of the detector's block in HBM; a crop_fn uploads the cropped image: same boxes, same counts
    a = CircuitPipeline(det, seg, tr, seg_batch=2, crop=True, reclassify=True).run_batch(images, "learned")
    b = CircuitPipeline(det, seg, tr, seg_batch=2, crop_fn=lambda im, bb: crop_image_and_adjust_bboxes(im, bb, padding=80), reclassify=True).run_batch(images, "learned")
    for (_, ra), (_, rb) in zip(a, b):
        assert ra["bboxes"] == rb["bboxes"] and ra["terminal_connections"] == rb["terminal_connections"] and ra["image"].shape == rb["image"].shape
    assert any(ra["terminal_connections"] for _, ra in a)
