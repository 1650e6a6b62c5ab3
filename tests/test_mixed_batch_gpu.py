"""Mixed-size image batches on the GPU: the ragged letterbox (cvmi_letterbox_ragged) against the oracle and against cvmi_letterbox per image, the
segmenter transform from a packed block (cvmi_sam2_transform_srcs) against transforming each crop, `YOLO.predict` on a list of differently
sized images (ultralytics: every image to the imgsz x imgsz square, one batch), and `CircuitPipeline(mixed_batch=True)`."""

import numpy as np
import pytest
import torch

from circuitvision_amd import _lib
from circuitvision_amd._lib import BF16, F16, F32
from circuitvision_amd.detector import YOLO, PackedImages, letterbox_geometry, letterbox_rows, pack_layout
from circuitvision_amd.pipeline import CircuitPipeline
from circuitvision_amd.sam2_infer import SAM2Transforms
from helpers import assert_same_detections, save_converted_yolo
from oracle import nms as onms
from oracle import preprocess as opre
from oracle.yolo11 import YOLO11
from synth import calibrated_yolo_params, circuit_image

pytestmark = pytest.mark.gpu

TD = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}


# ---- kernel 1 ---------------------------------------------------------------------------------------------------------------------------
def _rand_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _pack(images, lead=0):
    """images back to back behind `lead` spare bytes -> (u8 device buffer, byte offsets)."""
    offsets, total = pack_layout([im.shape[:2] for im in images])
    flat = np.zeros(lead + total, dtype=np.uint8)
    for im, off in zip(images, offsets):
        flat[lead + off:lead + off + im.size] = im.reshape(-1)
    return torch.from_numpy(flat).cuda(), [lead + o for o in offsets]


def _s2d_to_hwc(x, H, W):
    return x[..., :12].reshape(H // 2, W // 2, 2, 2, 3).permute(0, 2, 1, 3, 4).reshape(H, W, 3)


def _ragged(lib, data, rows, B, S, dtype, s2d, fill=7.0):
    dst = torch.full((B, S // 2, S // 2, 16) if s2d else (B, S, S, 3), fill, dtype=TD[dtype], device="cuda")
    _lib.check(lib.cvmi_letterbox_ragged(data.data_ptr(), data.numel(), rows.ctypes.data, B, dst.data_ptr(), dst[0].numel(), S, S, dtype, s2d, None),
               "letterbox_ragged")
    return dst


def _single(lib, img_dev, r, S, dtype, s2d):
    dst = torch.full((S // 2, S // 2, 16) if s2d else (S, S, 3), 7.0, dtype=TD[dtype], device="cuda")
    _lib.check(lib.cvmi_letterbox(img_dev.data_ptr(), int(r["H"]), int(r["W"]), dst.data_ptr(), S, S, int(r["new_h"]), int(r["new_w"]), int(r["top"]),
                                  int(r["left"]), dtype, s2d, None), "letterbox")
    return dst


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("S", [32, 64, 160])
def test_ragged_letterbox_is_bit_identical_to_the_oracle_and_to_the_single_image_kernel(S, dtype, lead):
    """One launch over a one-row and a one-column source, two sources whose canvas is mostly padding (padding-only tiles), an identity copy,
    an up-scaling source (64 x 64 at 160) and two general ones; canvas smaller than a tile (32), one whole column tile (64), a partial
    column tile (160 = 64 + 64 + 32); lead = 1: every image starts at an odd byte offset.  Both output forms, zero channels 12..15 included."""
    lib = _lib.load()
    shapes = [(1, 50), (50, 1), (37, 1000), (1000, 37), (S, S), (64, 64), (300, 200), (493, 712)]
    images = [_rand_image(h, w, 10 + i) for i, (h, w) in enumerate(shapes)]
    data, offsets = _pack(images, lead)
    assert lead == 0 or all(o % 2 == 1 for o in offsets[:2])
    rows = letterbox_rows(shapes, offsets, S)
    B = len(images)
    for s2d in (0, 1):
        got = _ragged(lib, data, rows, B, S, dtype, s2d)
        torch.cuda.synchronize()
        for b, im in enumerate(images):
            hwc = _s2d_to_hwc(got[b], S, S) if s2d else got[b]
            want = torch.from_numpy(np.ascontiguousarray(opre.letterbox(im, S, auto=False)[..., ::-1]).astype(np.float32) / 255.0).to(TD[dtype])
            assert want.shape == (S, S, 3) and torch.equal(hwc.cpu(), want), (S, dtype, s2d, b, shapes[b])
            one = _single(lib, torch.from_numpy(im).cuda(), rows[b], S, dtype, s2d)
            assert torch.equal(got[b], one), (S, dtype, s2d, b, shapes[b])
            if s2d:
                assert float(got[b][..., 12:].float().abs().max()) == 0.0, "channels 12..15 are written, as zeros"


def test_ragged_letterbox_65_images_take_two_launches():
    lib = _lib.load()
    S = 32
    shapes = [(1 + b % 7, 1 + (3 * b) % 11) for b in range(64)] + [(9, 5)]
    images = [_rand_image(h, w, 100 + i) for i, (h, w) in enumerate(shapes)]
    data, offsets = _pack(images)
    assert any(o % 2 for o in offsets)
    rows = letterbox_rows(shapes, offsets, S)
    for dtype in (F32, F16):
        for s2d in (0, 1):
            got = _ragged(lib, data, rows, 65, S, dtype, s2d)
            for b, im in enumerate(images):
                assert torch.equal(got[b], _single(lib, torch.from_numpy(im).cuda(), rows[b], S, dtype, s2d)), (dtype, s2d, b)


def test_ragged_letterbox_refuses_a_bad_row_and_launches_nothing():
    lib = _lib.load()
    S = 32
    shapes = [(5, 7)] * 66
    images = [_rand_image(5, 7, 200 + i) for i in range(66)]
    data, offsets = _pack(images)
    for bad_row in (2, 65):                                              # 65: in the second launch's table -- the first must not run either
        rows = letterbox_rows(shapes, offsets, S)
        rows[bad_row]["left"] = S - int(rows[bad_row]["new_w"]) + 1       # left + new_w > out_w
        dst = torch.full((66, S // 2, S // 2, 16), 7.0, device="cuda")
        rc = lib.cvmi_letterbox_ragged(data.data_ptr(), data.numel(), rows.ctypes.data, 66, dst.data_ptr(), dst[0].numel(), S, S, F32, 1, None)
        assert rc != 0 and (b"row %d:" % bad_row) in lib.cvmi_last_error(), lib.cvmi_last_error()
        torch.cuda.synchronize()
        assert bool((dst == 7.0).all()), "nothing was launched"
    rows = letterbox_rows(shapes, offsets, S)
    rows[1]["src_byte_offset"] = data.numel() - 5 * 7 * 3 + 1             # the image would leave the source buffer
    dst = torch.full((66, S, S, 3), 7.0, device="cuda")
    rc = lib.cvmi_letterbox_ragged(data.data_ptr(), data.numel(), rows.ctypes.data, 66, dst.data_ptr(), dst[0].numel(), S, S, F32, 0, None)
    assert rc != 0 and b"row 1:" in lib.cvmi_last_error()
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())


# ---- kernel 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_transform_from_a_packed_block_is_bit_identical_to_transforming_crops(dtype):
    """`forward_windows(PackedImages, windows)` (cvmi_sam2_transform_srcs) == `forward_batch([crop])` per image, for three sources of
    different sizes (the third at an odd byte offset): a border window, a one-pixel strip, the whole image, then a 6x down-scaling, a far
    corner and an up-scaling window; with and without the channel swap.  A ragged `forward_batch` takes the same kernel."""
    R = 256
    tr = SAM2Transforms(resolution=R, mask_threshold=0, max_hole_area=0, max_sprinkle_area=0)
    imgs = [circuit_image(700, 1500, seed=60), circuit_image(333, 517, seed=61), circuit_image(400, 900, seed=62)]
    packed = PackedImages.upload(imgs)
    assert packed.offsets[2] % 2 == 1 and torch.equal(packed.image(1).cpu(), torch.from_numpy(imgs[1]))
    window_sets = ([(0, 0, 300, 200), (10, 150, 500, 151), None], [(7, 3, 1493, 697), (218, 134, 517, 333), (200, 100, 260, 180)])
    for swap in (False, True):
        for wins in window_sets:
            out = torch.empty(3, R, R, 3, dtype=TD[dtype], device="cuda")
            tr.forward_windows(packed, wins, swap_rb=swap, out=out, out_dtype=dtype)
            for b, (im, w) in enumerate(zip(imgs, wins)):
                crop = im if w is None else np.ascontiguousarray(im[w[1]:w[3], w[0]:w[2]])
                ref = torch.empty(1, R, R, 3, dtype=TD[dtype], device="cuda")
                tr.forward_batch([crop], swap_rb=swap, out=ref, out_dtype=dtype)
                assert torch.equal(out[b], ref[0]), (dtype, swap, b, w)
        whole = torch.empty(3, R, R, 3, dtype=TD[dtype], device="cuda")
        tr.forward_batch(imgs, swap_rb=swap, out=whole, out_dtype=dtype)  # ragged: the packed upload + one launch
        for b, im in enumerate(imgs):
            ref = torch.empty(1, R, R, 3, dtype=TD[dtype], device="cuda")
            tr.forward_batch([im], swap_rb=swap, out=ref, out_dtype=dtype)
            assert torch.equal(whole[b], ref[0]), (dtype, swap, b)
    x = tr.forward_windows(packed[1:], [None, (0, 0, 10, 10)])            # a slice, the torch-op form
    assert x.shape == (2, 3, R, R) and x.dtype == torch.float32
    assert torch.equal(x[0], tr.forward_batch([imgs[1]])[0])
    lib = _lib.load()
    rows = np.zeros(1, dtype=_lib.SAM2_SRC_ROW)
    rows[0] = (packed.offsets[1], 333, 517, 400, 0, 200, 100)              # leaves the image: refused, nothing launched
    rc = lib.cvmi_sam2_transform_srcs(packed.data.data_ptr(), packed.data.numel(), rows.ctypes.data, 1, x.data_ptr(), R, F32, 0, None)
    assert rc != 0 and b"leaves the" in lib.cvmi_last_error()
    rows[0] = (packed.data.numel() - 10, 333, 517, 0, 0, 517, 333)         # the image leaves the buffer
    rc = lib.cvmi_sam2_transform_srcs(packed.data.data_ptr(), packed.data.numel(), rows.ctypes.data, 1, x.data_ptr(), R, F32, 0, None)
    assert rc != 0 and b"source buffer" in lib.cvmi_last_error()
    with pytest.raises(ValueError):
        tr.forward_windows(packed, [None])


# ---- detector ---------------------------------------------------------------------------------------------------------------------------
ABC = [(360, 500), (500, 360), (200, 200)]


@pytest.fixture(scope="module")
def mixed_detectors(tmp_path_factory):
    """Weights calibrated on the three images as the square canvas shows them; the f32 and f16 detectors and the oracle network."""
    images = [circuit_image(h, w, seed=40 + i) for i, (h, w) in enumerate(ABC)]
    x = torch.cat([_oracle_input(im) for im in images])
    params = calibrated_yolo_params("n", 62, 3, x)
    path = save_converted_yolo(str(tmp_path_factory.mktemp("mixed") / "y.pt"), params, "n", 62)
    oracle = YOLO11("n", 62).eval()
    oracle.load_state_dict(params.state_dict(), strict=True)
    return images, {dt: YOLO(path, dtype=dt) for dt in ("f32", "f16")}, oracle


def _oracle_input(im, imgsz=640):
    lb = opre.letterbox(im, imgsz, auto=False)
    return torch.from_numpy(np.ascontiguousarray(lb[..., ::-1].transpose(2, 0, 1)).astype(np.float32) / 255.0)[None]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_predict_takes_a_mixed_list_as_one_square_batch(mixed_detectors, dtype):
    """`predict([A, B, C])` with three sizes runs as ONE batch on the imgsz x imgsz canvas (it raised ValueError before), and Results[i] equals
    slot i of `predict([X, X, X], rect=False)` bit for bit: same plan, same slot, same canvas; the per-image scale_boxes is in the equality."""
    images, dets, _ = mixed_detectors
    det = dets[dtype]
    plans_before = set(det._plans)
    res = det.predict(images, verbose=False)
    assert len(res) == 3 and [r.orig_shape for r in res] == ABC and all(r.letterboxed_shape == (640, 640) for r in res)
    assert {k[:3] for k in set(det._plans) - plans_before} <= {(3, 640, 640)} and (3, 640, 640) in {k[:3] for k in det._plans}
    h = det.predict_async(images)
    again = h.result()
    moved = 0
    for i, im in enumerate(images):
        same = det.predict([im, im, im], verbose=False, rect=False)[i]
        assert torch.equal(res[i].boxes.data, same.boxes.data) and torch.equal(res[i].anchor_idx, same.anchor_idx), (dtype, i)
        assert torch.equal(res[i].boxes.data, again[i].boxes.data) and same.orig_shape == ABC[i]
        raw = h.det[i, :len(res[i]), :4]                                 # the plan's boxes, in canvas coordinates
        moved += len(res[i]) >= 20 and float((raw - res[i].boxes.xyxy).abs().max()) > 5.0
    assert max(len(r) for r in res) >= 20 and moved >= 1, [len(r) for r in res]
    assert {k[:3] for k in det._plans} == {k[:3] for k in plans_before} | {(3, 640, 640)}, "one plan serves every size"


def test_square_predict_matches_the_oracle_chain(mixed_detectors):
    """One image with rect=False, f32: oracle letterbox(auto=False) -> oracle network -> oracle NMS -> scale_boxes; identical anchors (or a
    checked threshold tie), 1e-3 on the confidences, 0.05 px on the boxes."""
    images, dets, oracle = mixed_detectors
    img = images[0]
    r = dets["f32"].predict(img, verbose=False, rect=False)[0]
    assert r.letterboxed_shape == (640, 640) and r.orig_shape == img.shape[:2]
    x = _oracle_input(img)
    with torch.no_grad():
        pred = oracle(x)
    ref, ref_idx = onms.yolo_nms(pred, 0.25, 0.7, 300, return_indices=True)
    ref, ref_idx = ref[0], ref_idx[0]
    unscaled = ref[:, :4].clone()
    ref[:, :4] = onms.scale_boxes((640, 640), ref[:, :4], img.shape[:2])
    assert ref.shape[0] >= 20 and float((ref[:, :4] - unscaled).abs().max()) > 5.0
    got_idx = r.anchor_idx.cpu().tolist()
    assert_same_detections("square predict f32", got_idx, ref_idx.tolist(), pred=pred[0])
    gm, rm = {a: i for i, a in enumerate(got_idx)}, {int(a): i for i, a in enumerate(ref_idx)}
    common = [a for a in got_idx if a in rm]
    assert len(common) >= 20
    gi, ri = [gm[a] for a in common], [rm[a] for a in common]
    assert r.boxes.cls[gi].tolist() == ref[ri, 5].tolist()
    np.testing.assert_allclose(r.boxes.conf[gi].numpy(), ref[ri, 4].numpy(), atol=1e-3)
    np.testing.assert_allclose(r.boxes.xyxy[gi].numpy(), ref[ri, :4].numpy(), atol=0.05)


def test_equal_shapes_with_rect_unset_keep_the_rectangle(mixed_detectors):
    images, dets, _ = mixed_detectors
    det = dets["f16"]
    im = images[0]
    nw, nh, top, bottom, left, right = letterbox_geometry(*im.shape[:2], 640)
    res = det.predict([im, im], verbose=False)
    assert all(r.letterboxed_shape == (nh + top + bottom, nw + left + right) == (480, 640) for r in res)
    h = det.predict_chunks_async([im, im, im], 2)
    assert [tuple(x.src.shape) for x in h] == [(2, 360, 500, 3), (1, 360, 500, 3)] and all(x.orig_shape == (360, 500) and x.orig_shapes is None for x in h)
    [x.result() for x in h]
    h = det.predict_chunks_async(images, 2)                             # mixed: PackedImages slices
    assert [len(x.src) for x in h] == [2, 1] and isinstance(h[0].src, PackedImages) and h[1].src.shapes == [ABC[2]] and h[0].orig_shapes == ABC[:2]
    assert torch.equal(h[1].src.image(0).cpu(), torch.from_numpy(images[2]))
    got = [r for x in h for r in x.result()]
    assert [r.orig_shape for r in got] == ABC


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------------
def _same_results(a, b, tag):
    for (i, ra), (j, rb) in zip(a, b):
        assert i == j and ra["bboxes"] == rb["bboxes"] and ra["crop_debug_info"] == rb["crop_debug_info"], (tag, i)
        assert np.array_equal(ra["image"], rb["image"]) and torch.equal(ra["mask"], rb["mask"]) and ra["extent"] == rb["extent"], (tag, i)
        assert torch.equal(ra["iou"], rb["iou"]), (tag, i)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_mixed_batch_cropped_chain_equals_the_generic_path_bit_for_bit(tmp_path, dtype):
    """The ragged image set of test_crop_gpu through `CircuitPipeline(mixed_batch=True, crop=True)` -- one packed upload, square detector
    chunks, the segmenter's windows read out of the packed block -- == the generic path (mixed detector batch, host crop, a transform per
    chunk of crops); once more with reclassify=True (its windows read out of the packed block too).  Only square plans, one per chunk size."""
    from circuitvision_amd.crop import crop_image_and_adjust_bboxes
    from test_crop_gpu import _setup
    images, det, yo, seg, tr, so, R = _setup(tmp_path, dtype=dtype)
    ragged = images[:3] + [circuit_image(260, 300, seed=77), circuit_image(340, 280, seed=78)]
    crop_fn = lambda im, bb: crop_image_and_adjust_bboxes(im, bb, padding=20)
    fast = CircuitPipeline(det, seg, tr, mixed_batch=True, crop=True, crop_padding=20, seg_batch=2)
    slow = CircuitPipeline(det, seg, tr, mixed_batch=True, seg_batch=2, crop_fn=crop_fn)
    a, b = fast.run_batch(ragged, "learned"), slow.run_batch(ragged, "learned")
    assert any("detector chunk" in k for k in fast.timings) and not any("enqueue" in k for k in slow.timings)
    _same_results(a, b, dtype)
    assert sum(len(r["bboxes"]) for _, r in a) >= 10, "the comparison is not about empty lists"
    # chunks of 2, 2, 1 images (fast) and one batch of 5 (generic): square plans only
    assert {k[:3] for k in det._plans} == {(2, 640, 640), (1, 640, 640), (5, 640, 640)}, sorted(k[:3] for k in det._plans)
    # reclassify: name the most frequent class 'terminal' so that the step has work
    ids = [bb["_yolo_class_id_temp"] for _, r in a for bb in r["bboxes"]]
    by_count = sorted(set(ids), key=lambda i: (-ids.count(i), i))
    other = by_count[1] if len(by_count) > 1 else (by_count[0] + 1) % len(det.names)
    det.names[by_count[0]], det.names[other] = "terminal", "voltage.dc"
    a = CircuitPipeline(det, seg, tr, mixed_batch=True, crop=True, crop_padding=20, seg_batch=2, reclassify=True).run_batch(ragged, "learned")
    b = CircuitPipeline(det, seg, tr, mixed_batch=True, seg_batch=2, crop_fn=crop_fn, reclassify=True).run_batch(ragged, "learned")
    _same_results(a, b, dtype + " reclassify")
    for (_, ra), (_, rb) in zip(a, b):
        assert ra["terminal_connections"] == rb["terminal_connections"]
    assert any(ra["terminal_connections"] for _, ra in a)
    assert {k[:3] for k in det._plans} == {(2, 640, 640), (1, 640, 640), (5, 640, 640)}


def test_mixed_batch_switch(tmp_path):
    """mixed_batch=True with device_glue=True is refused; mixed_batch=False (the default) still runs one detector batch per image size, each on
    its own rectangle; the uncropped overlapped path and `detect` hand the whole list to the detector when mixed_batch=True."""
    from test_crop_gpu import _setup
    images, det, yo, seg, tr, so, R = _setup(tmp_path, n_images=3, dtype="f16")
    ragged = images[:2] + [circuit_image(260, 300, seed=77), circuit_image(340, 280, seed=78)]
    with pytest.raises(ValueError, match="mixed_batch"):
        CircuitPipeline(det, seg, tr, crop=True, device_glue=True, mixed_batch=True)
    grouped = CircuitPipeline(det, seg, tr, crop=True, crop_padding=20, seg_batch=2)
    assert grouped.mixed_batch is False
    g = grouped.run_batch(ragged, "learned")
    assert any("detector chunk" in k for k in grouped.timings)
    # 300 x 420 -> 480 x 640 (two images: one chunk of 2), 260 x 300 -> 576 x 640, 340 x 280 -> 640 x 544: a plan per size, none square
    assert {k[:3] for k in det._plans} == {(2, 480, 640), (1, 576, 640), (1, 640, 544)}, sorted(k[:3] for k in det._plans)
    assert len(det._staging) == 3 and det._flat_staging[0] is None, "one staging buffer per size, the flat one untouched"
    det._plans.clear()
    over = CircuitPipeline(det, seg, tr, seg_batch=2, mixed_batch=True)
    o = over.run_batch(ragged, "learned")
    assert any(k.startswith("enqueue: detector") for k in over.timings) and {k[:3] for k in det._plans} == {(4, 640, 640)}
    d = CircuitPipeline(det, seg, tr, seg_batch=2, mixed_batch=True).detect(ragged)
    assert [r["bboxes"] for _, r in o] == d and {k[:3] for k in det._plans} == {(4, 640, 640)}
    assert [r["image"].shape for _, r in o] == [im.shape for im in ragged] and all(r["mask"].shape == im.shape[:2] for (_, r), im in zip(o, ragged))
    assert len(g) == len(o) == 4
