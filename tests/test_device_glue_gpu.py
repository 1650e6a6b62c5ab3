"""The device-resident glue on the GPU (csrc/glue_ops.hip stage2_crop_kernel, the device-window forms of the segmenter's transform and mask
post-processing, `CircuitPipeline(device_glue=True)`): every comparison is exact equality -- against the vectors recorded from the reference's
own code (tests/golden/nms_stage2.json, crop.json), against the host chain it restates, and against the host-table kernels."""
import json
import os

import numpy as np
import pytest
import torch

from circuitvision_amd import _lib, glue
from circuitvision_amd._lib import BF16, F16, F32
from circuitvision_amd.crop import adjust_bboxes, crop_window
from circuitvision_amd.detector import non_max_suppression_by_confidence, scale_boxes
from circuitvision_amd.pipeline import CircuitPipeline
from circuitvision_amd.sam2_infer import SAM2Transforms

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NMS_CASES = json.load(open(os.path.join(GOLD, "nms_stage2.json")))["cases"]
CROP_CASES = json.load(open(os.path.join(GOLD, "crop.json")))["cases"]


def _run(lists, names, hw, padding, iou, lb_hw=None, max_det=300):
    """lists: per image [(x1, y1, x2, y2, conf, class id)] in letterboxed coordinates -> (det, count) host tensors and the kernel's outputs."""
    B = len(lists)
    det = torch.zeros(B, max_det, 6, dtype=torch.float32)
    for b, rows in enumerate(lists):
        if rows:
            det[b, :len(rows)] = torch.tensor(rows, dtype=torch.float64).to(torch.float32)
    count = torch.tensor([len(r) for r in lists], dtype=torch.int32)
    flags = torch.from_numpy(glue.class_flags(names)).cuda()
    out = glue.stage2_crop(det.cuda(), count.cuda(), lb_hw or hw, hw, flags, padding, iou)
    torch.cuda.synchronize()
    return det, count, out


def _rows(boxes, ids):
    return [(b["xmin"], b["ymin"], b["xmax"], b["ymax"], b["confidence"], ids[b["class"]]) for b in boxes]


def test_stage2_nms_equals_the_reference_vectors():
    """nms_stage2.json, all 18 cases (gain 1, no pad, 640 x 640): the kept uids, in order, are the reference's kept_by_confidence."""
    assert len(NMS_CASES) == 18
    names = sorted({b["class"] for c in NMS_CASES for b in c["boxes"]})
    ids = {nm: i for i, nm in enumerate(names)}
    for c in NMS_CASES:                                                    # preconditions of running these vectors through f32 detections
        conf = np.array([b["confidence"] for b in c["boxes"]], dtype=np.float64)
        assert np.array_equal(np.argsort(-conf, kind="stable"), np.argsort(-conf.astype(np.float32), kind="stable")), c["name"]
        assert all(0 <= b[k] <= 640 and b[k] == int(b[k]) for b in c["boxes"] for k in ("xmin", "ymin", "xmax", "ymax")), c["name"]
    for thr in sorted({c["iou_threshold"] for c in NMS_CASES}):
        cases = [c for c in NMS_CASES if c["iou_threshold"] == thr]
        det, count, out = _run([_rows(c["boxes"], ids) for c in cases], names, (640, 640), 80, thr)
        got = glue.to_host(det, count, out, names, (640, 640), uids=[[b["persistent_uid"] for b in c["boxes"]] for c in cases])
        for c, (bbs, _shifted, _win, _info) in zip(cases, got):
            want = [k["persistent_uid"] if isinstance(k, dict) else k for k in c["kept_by_confidence"]]
            assert [b["persistent_uid"] for b in bbs] == want, c["name"]
            by_uid = {b["persistent_uid"]: b for b in c["boxes"]}
            assert all((b["xmin"], b["ymin"], b["xmax"], b["ymax"], b["class"]) == tuple(by_uid[b["persistent_uid"]][k] for k in ("xmin", "ymin", "xmax", "ymax", "class"))
                       for b in bbs), c["name"]


def test_crop_window_equals_the_reference_vectors():
    """crop.json through the kernel (no stage-2 pass: the vectors' boxes were never sorted), one launch per image size and padding: every
    expected key to_host produces equals the vector -- window, shifted boxes, decision, the text boxes that grew the window.  The one case
    left to the host mirror's CPU test is float_coordinates: the pipeline only ever hands the kernel rounded integers."""
    skipped = [c["name"] for c in CROP_CASES if c["name"] == "float_coordinates"]
    cases = [c for c in CROP_CASES if c["name"] != "float_coordinates"]
    assert skipped == ["float_coordinates"] and len(cases) == len(CROP_CASES) - 1 == 33
    names = sorted({b["class"] for c in cases for b in c["boxes"]})
    ids = {nm: i for i, nm in enumerate(names)}
    groups = {}
    for c in cases:
        assert all(b[k] == int(b[k]) for b in c["boxes"] for k in ("xmin", "ymin", "xmax", "ymax")), c["name"]
        groups.setdefault((c["height"], c["width"], c["padding"]), []).append(c)
    tup = lambda v: None if v is None else list(v)
    for (H, W, pad), cs in groups.items():
        lists = [[(b["xmin"], b["ymin"], b["xmax"], b["ymax"], float(np.float32(b.get("confidence", 0.5))), ids[b["class"]]) for b in c["boxes"]] for c in cs]
        det, count, out = _run(lists, names, (H, W), pad, -1.0)
        got = glue.to_host(det, count, out, names, (H, W), uids=[[b["persistent_uid"] for b in c["boxes"]] for c in cs])
        wins = out.window.cpu().tolist()
        for c, (bbs, shifted, win, info), wdev in zip(cs, got, wins):
            e, nm = c["expected"], c["name"]
            assert [b["persistent_uid"] for b in bbs] == [b["persistent_uid"] for b in c["boxes"]], nm        # list order kept
            for key in ("crop_applied", "reason_for_no_crop", "crop_decision_source", "clustering_proximity_threshold", "num_clusters_found",
                        "num_component_type_bboxes", "num_text_type_bboxes"):
                assert info[key] == e[key], (nm, key)
            for key in ("final_crop_window_abs", "cropped_image_dims", "original_image_dims", "crop_basis_bbox_before_padding", "window_after_main_padding"):
                assert tup(info[key]) == e[key], (nm, key)
            assert info["padding_value"] == pad and info["num_total_yolo_bboxes"] == len(c["boxes"])
            mc = info["main_cluster_info"]
            assert (mc["num_elements"] if mc else None) == e["main_cluster_num_elements"], nm
            assert (mc["example_uid"] if mc else None) == e["main_cluster_example_uid"], nm
            assert [t["uid"] for t in info["text_bboxes_that_expanded_crop"]] == e["text_uids_that_expanded_crop"], nm
            assert (list(win) if win else None) == (e["final_crop_window_abs"] if e["crop_applied"] else None), nm
            assert [[b["persistent_uid"], b["xmin"], b["ymin"], b["xmax"], b["ymax"]] for b in shifted] == e["boxes"], nm
            x0, y0, x1, y1 = win or (0, 0, W, H)
            assert [y1 - y0, x1 - x0, 3] == e["image_shape"] and wdev == [x0, y0, x1 - x0, y1 - y0], nm
            # the whole dict against the host mirror, too
            hwin, hinfo = crop_window(c["boxes"], (H, W), pad)
            assert info == hinfo and win == hwin, nm


SEAM_CLASSES = ["resistor", "capacitor.unpolarized", "diode", "gnd", "junction", "junction", "text", "text", "text", "crossover", "vss", "explanatory", "circuit"]
SEAM_SEED = 0


def _seam_images(seed, W=1200, H=900):
    """Counts at the workgroup's seams (one thread per box up to 256, two above), boxes in three clusters, a class mix with text and junctions."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (0, 1, 255, 256, 257, 300):
        cx, cy = rng.integers(100, W - 100, size=3), rng.integers(100, H - 100, size=3)
        rows = []
        for _ in range(n):
            k = int(rng.integers(0, 3))
            x0 = int(np.clip(cx[k] + rng.normal(0, 60), 0, W - 1))
            y0 = int(np.clip(cy[k] + rng.normal(0, 60), 0, H - 1))
            w, h = int(rng.integers(0, 90)), int(rng.integers(0, 90))
            conf = float(np.float32(rng.integers(1, 64) / 64.0))           # few distinct values: ties keep their list order
            rows.append((x0, y0, min(W, x0 + w), min(H, y0 + h), conf, int(rng.integers(0, len(SEAM_CLASSES)))))
        out.append(rows)
    return out


def _host_chain(rows, names, hw, padding, iou):
    bbs = []
    for x0, y0, x1, y1, conf, ci in rows:
        nm = names[ci]
        bbs.append({"class": nm, "_yolo_class_id_temp": ci, "confidence": conf, "xmin": x0, "ymin": y0, "xmax": x1, "ymax": y1,
                    "persistent_uid": f"{nm}_{x0}_{y0}_{x1}_{y1}"})
    kept = non_max_suppression_by_confidence(bbs, iou_threshold=iou)
    win, info = crop_window(kept, hw, padding)
    return kept, adjust_bboxes(kept, win), win, info


def test_workgroup_seams_equal_the_host_chain():
    """0, 1, 255, 256, 257 and 300 boxes in one launch == non_max_suppression_by_confidence + crop_window + adjust_bboxes on the host."""
    hw, pad, iou = (900, 1200), 20, 0.6
    lists = _seam_images(SEAM_SEED)
    want = [_host_chain(rows, SEAM_CLASSES, hw, pad, iou) for rows in lists]
    assert sum(w[2] is not None for w in want) >= 3, "the seed must give real windows on at least half of the images"
    assert any(len(w[0]) < len(rows) for w, rows in zip(want, lists)) and any(w[3]["text_bboxes_that_expanded_crop"] for w in want)
    det, count, out = _run(lists, SEAM_CLASSES, hw, pad, iou)
    got = glue.to_host(det, count, out, SEAM_CLASSES, hw)
    assert out.kept_count.cpu().tolist() == [len(w[0]) for w in want]
    for n, g, w in zip((0, 1, 255, 256, 257, 300), got, want):
        assert g[0] == w[0] and g[1] == w[1] and g[2] == w[2] and g[3] == w[3], n


def test_scale_boxes_and_rounding_equal_the_host():
    """A 900 x 1200 original under a 480 x 640 letterbox (gain 8/15): 300 boxes per image, with coordinates that land on .5 after the division
    and coordinates outside the clamp -- the integer boxes are np.rint(scale_boxes(...)), bit for bit."""
    lb, hw = (480, 640), (900, 1200)
    g = torch.Generator().manual_seed(11)
    det = torch.zeros(2, 300, 6)
    det[..., :4] = torch.rand(2, 300, 4, generator=g) * 700 - 30            # some outside [0, 640] x [0, 480]
    det[0, :150, :4] = (torch.arange(600, dtype=torch.float32).reshape(150, 4) * 2 + 1) * (4.0 / 15.0)      # (m + 1/2) * gain
    det[..., 4] = torch.rand(2, 300, generator=g)
    want = scale_boxes(lb, det[..., :4].reshape(-1, 4), hw).reshape(2, 300, 4)
    frac = want - want.floor()
    assert int((frac == 0.5).sum()) >= 20, "the inputs must include values that land on .5"
    assert int(((want == 0) | (want == 1200) | (want == 900)).sum()) >= 20, "... and values the clamp catches"
    count = torch.tensor([300, 300], dtype=torch.int32)
    flags = torch.zeros(1, dtype=torch.uint8, device="cuda")
    out = glue.stage2_crop(det.cuda(), count.cuda(), lb, hw, flags, 80, -1.0)
    assert np.array_equal(out.boxes.cpu().numpy(), np.rint(want.numpy().astype(np.float64)).astype(np.int32))
    assert out.kept_count.cpu().tolist() == [300, 300] and out.kept_idx.cpu()[0].tolist() == list(range(300))


WINDOWS = [(0, 0, 128, 96), (10, 5, 60, 40), (67, 31, 61, 65)]             # {x0, y0, w, h} of a 96 x 128 image: the whole image, inside, to the corner


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_transform_from_device_windows_equals_the_host_table_form(dtype):
    """cvmi_sam2_transform_rects_dev (windows read from device memory) == cvmi_sam2_transform_rects (windows in the kernel arguments)."""
    lib = _lib.load()
    R, H, W = 64, 96, 128
    src = torch.randint(0, 256, (3, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).cuda()
    rects = np.array(WINDOWS, dtype=np.int32)
    rects_dev = torch.from_numpy(rects).cuda()
    td = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}[dtype]
    for swap in (0, 1):
        a = torch.zeros(3, R, R, 3, dtype=td, device="cuda")
        b = torch.ones(3, R, R, 3, dtype=td, device="cuda")
        _lib.check(lib.cvmi_sam2_transform_rects(src.data_ptr(), H * W * 3, H, W, rects.ctypes.data, 3, a.data_ptr(), R, dtype, swap, None), "host table")
        _lib.check(lib.cvmi_sam2_transform_rects_dev(src.data_ptr(), H * W * 3, H, W, rects_dev.data_ptr(), 3, b.data_ptr(), R, dtype, swap, None), "device table")
        torch.cuda.synchronize()
        assert torch.equal(a, b), swap
    assert lib.cvmi_sam2_transform_rects_dev(src.data_ptr(), H * W * 3, H, W, None, 3, b.data_ptr(), R, dtype, 0, None) != 0


def test_masks_return_to_device_windows_equal_the_host_sizes_form():
    """cvmi_mask_postprocess_rects_dev (sizes from the device windows, fixed plane stride) == cvmi_mask_postprocess_sizes (host sizes, packed)."""
    lib = _lib.load()
    tr = SAM2Transforms(resolution=64, mask_threshold=0, max_hole_area=0, max_sprinkle_area=0)
    H, W = 96, 128
    logits = (torch.randn(3, 1, 64, 64, generator=torch.Generator().manual_seed(6)) * 3 - 1.0).cuda()
    logits[1] = -4.0                                                        # an empty mask
    masks, ext = tr.postprocess_to_masks_sized(logits, [(h, w) for _, _, w, h in WINDOWS])
    rects_dev = torch.tensor(WINDOWS, dtype=torch.int32).cuda()
    u8 = torch.full((3, H * W), 7, dtype=torch.uint8, device="cuda")
    ext2 = torch.empty(3, 4, dtype=torch.int32, device="cuda")
    _lib.check(lib.cvmi_mask_postprocess_rects_dev(logits.data_ptr(), 3, 64, 64, rects_dev.data_ptr(), H * W, float(tr.mask_threshold), u8.data_ptr(),
                                                   ext2.data_ptr(), None), "mask_postprocess_rects_dev")
    torch.cuda.synchronize()
    assert torch.equal(ext, ext2)
    for n, (_, _, w, h) in enumerate(WINDOWS):
        assert torch.equal(u8[n, :h * w].view(h, w), masks[n]), n
        assert bool((u8[n, h * w:] == 7).all()), "nothing is written past a plane's own pixels"


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    det = torch.zeros(1, glue.MAX_DET + 1, 6, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    flags = torch.zeros(4, dtype=torch.uint8, device="cuda")
    o = glue.GlueOutputs(1, glue.MAX_DET + 1, "cuda")
    lib.cvmi_last_kernel()                                                  # (read-and-clear)

    def call(max_det, kept_idx):
        return lib.cvmi_stage2_crop(det.data_ptr(), count.data_ptr(), 1, max_det, 640, 640, 1.0, 0, 0, 0.6, 80, flags.data_ptr(), 4, kept_idx,
                                    o.kept_count.data_ptr(), o.boxes.data_ptr(), o.adj_boxes.data_ptr(), o.window.data_ptr(), o.info.data_ptr(), None)
    assert call(glue.MAX_DET + 1, o.kept_idx.data_ptr()) != 0
    assert b"max_det" in lib.cvmi_last_error() and lib.cvmi_last_kernel() == b""
    assert call(300, None) != 0
    assert b"null pointer" in lib.cvmi_last_error() and lib.cvmi_last_kernel() == b""
    with pytest.raises(_lib.CvmiError):
        glue.stage2_crop(det, count, (640, 640), (640, 640), flags, 80, 0.6)
    assert call(300, o.kept_idx.data_ptr()) == 0 and lib.cvmi_last_kernel() == b"stage2_crop_kernel"
    torch.cuda.synchronize()


def _same(a, b, path=""):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), path
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (path, list(a), list(b) if isinstance(b, dict) else b)
        for k in a:
            _same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    else:
        assert a == b and type(a) is type(b), (path, a, b)


def test_pipeline_with_device_glue_equals_the_host_glue(tmp_path):
    """Five 900 x 1200 images, crop_padding 80, seg_batch 2 (three chunks, the last one short): device_glue=True == False on every key --
    boxes, windows, crop_debug_info, images, masks, extents, IoU predictions -- and again with terminal reclassification and node analysis."""
    from test_crop_gpu import _setup
    images, det, _yo, seg, tr, _so, _R = _setup(tmp_path, hw=(900, 1200))
    for kw in ({}, {"reclassify": True, "nodes": "connections"}):
        host = CircuitPipeline(det, seg, tr, crop=True, crop_padding=80, seg_batch=2, **kw)
        dev = CircuitPipeline(det, seg, tr, crop=True, crop_padding=80, seg_batch=2, device_glue=True, **kw)
        a, b = host.run_batch(images, "learned"), dev.run_batch(images, "learned")
        assert any("glue kernel" in k for k in dev.timings) and not any("glue kernel" in k for k in host.timings)
        assert len(a) == len(b) == 5
        for (i, ra), (j, rb) in zip(a, b):
            assert i == j
            _same(ra, rb, f"image {i}")
        assert any(r["window"] is not None and (r["window"][2] - r["window"][0], r["window"][3] - r["window"][1]) != (1200, 900) for _, r in b)
        assert all(len(r["bboxes"]) >= 1 for _, r in b)
