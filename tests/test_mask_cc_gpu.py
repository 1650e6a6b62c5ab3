"""Hole and sprinkle removal on the GPU (csrc/mask_cc.hip: tile / seam / flatten / apply) through `get_connected_components`,
`SAM2Transforms.fill_small_regions`, the post-process methods and `CircuitPipeline`, against tests/mask_cc_ref.py (scipy).  Every comparison
is exact: labels and areas are integers, filled logits are copies of the input or one of two f32 constants."""
import numpy as np
import pytest
import torch

import mask_cc_ref as ref
from circuitvision_amd import _lib
from circuitvision_amd.sam2_infer import MASK_CC_TILE as T
from circuitvision_amd.sam2_infer import SAM2Transforms, get_connected_components
from test_mask_cc_cpu import HOLE_PAIR, RING, SIZES

pytestmark = pytest.mark.gpu

BIG = (2 * T + 1, 3 * T - 1)
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (T, T), (T - 1, T + 1), (T + 1, T - 1), BIG, (200, 328)]
DENSITIES = (0.05, 0.4, 0.5, 0.6, 0.95)


def gpu_components(fg):
    """bool [N, h, w] -> labels, areas int32 [N, h, w] over both phases: get_connected_components on the mask (bool) and on its complement (u8)"""
    m = torch.from_numpy(np.ascontiguousarray(fg))[:, None].cuda()
    l1, c1 = get_connected_components(m)
    l0, c0 = get_connected_components((~m).to(torch.uint8))
    for t_ in (l1, c1, l0, c0):
        assert t_.dtype == torch.int32 and t_.shape == m.shape
    assert not (l1[~m].any() or c1[~m].any() or l0[m].any() or c0[m].any())          # upstream's contract: 0 on the background
    return (l1 + l0)[:, 0].cpu().numpy(), (c1 + c0)[:, 0].cpu().numpy()


def check_components(fg):
    fg = np.asarray(fg, dtype=bool)
    lab, area = gpu_components(fg)
    rl, ra, _ = ref.components(np.where(fg, 1.0, 0.0).astype(np.float32), 0.5)
    assert np.array_equal(lab, rl)
    assert np.array_equal(area, ra)
    return lab, area


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_plane_sizes(shape, N):
    rng = np.random.RandomState(shape[0] * 1000 + shape[1] + N)
    check_components(rng.rand(N, *shape) < 0.5)


def _serpentine(h, w):
    m = np.zeros((h, w), dtype=bool)
    m[0::2] = True                                                         # full rows, joined alternately at the right and the left end
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = True
    return m


def _rings(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.minimum(np.minimum(yy, h - 1 - yy), np.minimum(xx, w - 1 - xx)) % 2 == 0


def _staircases(h, w):
    """single diagonal links through the four-tile corner points: the main diagonal, and anti-diagonals through (T, T), (2T, T), (T, 2T)"""
    a, b = np.zeros((h, w), dtype=bool), np.zeros((h, w), dtype=bool)
    for i in range(min(h, w)):
        a[i, i] = True
    for c in (2 * T - 1, 3 * T - 1):
        for y in range(h):
            if 0 <= c - y < w:
                b[y, c - y] = True
    return np.stack([a, b])


def _seam_pairs(h, w):
    m = np.zeros((h, w), dtype=bool)
    m[10, T - 1] = m[9, T] = True                                          # joined only by the NE diagonal across a vertical seam
    m[T, 10] = m[T - 1, 9] = True                                          # joined only by the NW diagonal across a horizontal seam
    m[2 * T - 1, 2 * T - 1] = m[2 * T, 2 * T] = True                         # and by the diagonal of a four-tile corner
    m[T - 1, 2 * T] = m[T, 2 * T - 1] = True                                # ... and its other diagonal
    return m


def _plane_boundary(h, w):
    m = np.zeros((2, h, w), dtype=bool)
    m[0, h - 1, 5:40] = m[1, 0, 5:40] = True
    return m


def _constructed():
    h, w = BIG
    yy, xx = np.mgrid[0:h, 0:w]
    return {"all_foreground": np.ones((1, h, w), dtype=bool), "all_background": np.zeros((1, h, w), dtype=bool),
            "checkerboard": ((yy + xx) % 2 == 0)[None], "serpentine_h": _serpentine(h, w)[None], "serpentine_v": _serpentine(w, h).T[None],
            "staircases": _staircases(h, w), "seam_pairs": _seam_pairs(h, w)[None], "rings": _rings(h, w)[None], "plane_boundary": _plane_boundary(h, w)}


CONSTRUCTED = _constructed()


@pytest.mark.parametrize("name", sorted(CONSTRUCTED))
def test_constructed_planes(name):
    fg = CONSTRUCTED[name]
    lab, area = check_components(fg)
    h, w = BIG
    if name == "checkerboard":
        assert sorted(np.unique(lab).tolist()) == [1, 2]
    if name.startswith("serpentine"):                                      # one long component through every tile
        assert np.unique(lab[fg]).tolist() == [1] and np.unique(area[fg]).tolist() == [int(fg.sum())]
    if name == "staircases":
        assert np.unique(lab[0][fg[0]]).tolist() == [1] and np.unique(area[0][fg[0]]).tolist() == [min(h, w)]
        assert len(np.unique(lab[1][fg[1]])) == 2
    if name == "seam_pairs":
        assert (area[fg] == 2).all() and len(np.unique(lab[fg])) == 4
    if name == "plane_boundary":
        assert (area[fg] == 35).all() and lab[0][fg[0]][0] == 1 + (h - 1) * w + 5 and lab[1][fg[1]][0] == 1 + 5


@pytest.mark.parametrize("density", DENSITIES)
def test_random_planes(density):
    rng = np.random.RandomState(int(density * 100))
    check_components(rng.rand(3, 200, 328) < density)


def _logits(fg, t, seed):
    """f32 logits with the foreground `fg` under threshold t; a share of the background is exactly t"""
    rng = np.random.RandomState(seed)
    mag = (rng.rand(*fg.shape) * 5 + 0.125).astype(np.float32)
    x = np.where(fg, np.float32(t) + mag, np.float32(t) - mag).astype(np.float32)
    x[~fg & (rng.rand(*fg.shape) < 0.25)] = np.float32(t)
    x[tuple(np.argwhere(~fg)[0])] = np.float32(t)
    assert ((x > np.float32(t)) == fg).all() and (x == np.float32(t)).any()
    return x


def check_fill(x, t):
    """hole only, sprinkle only and both, with limits 1, 8 and 2.5; the input stays as it was"""
    dev = torch.from_numpy(x)[:, None].cuda()
    keep = dev.clone()
    for limit in (1, 8, 2.5):
        for hole, sprinkle in ((limit, 0), (0, limit), (limit, limit)):
            y = SAM2Transforms(64, t, hole, sprinkle).fill_small_regions(dev)
            assert y is not dev and y.shape == dev.shape and y.dtype == torch.float32
            assert np.array_equal(y[:, 0].cpu().numpy(), ref.fill_small(x, t, hole, sprinkle)), (limit, hole, sprinkle)
    assert torch.equal(dev, keep)


@pytest.mark.parametrize("t", [0.0, 0.37])
@pytest.mark.parametrize("density", DENSITIES)
def test_fill_on_random_planes(density, t):
    rng = np.random.RandomState(int(density * 100) + 7)
    check_fill(_logits(rng.rand(3, 200, 328) < density, t, 11), t)


@pytest.mark.parametrize("t", [0.0, 0.37])
def test_fill_on_hand_cases(t):
    for case in (RING, HOLE_PAIR, SIZES):
        check_fill(_logits(case > 0, t, 3), t)
    x = _logits(RING > 0, t, 3)
    y = SAM2Transforms(64, t, 8, 8).fill_small_regions(torch.from_numpy(x)[None].cuda())[0].cpu().numpy()
    assert (y[RING > 0] == np.float32(t) - np.float32(10)).all() and y[0, 2, 2] == np.float32(t) + np.float32(10)      # deleted ring, filled centre


def test_zero_areas_are_the_old_path():
    lib = _lib.load()
    rng = np.random.RandomState(5)
    m = torch.from_numpy(rng.randn(3, 1, 96, 96).astype(np.float32)).cuda()
    tr = SAM2Transforms(96, 0.0, 0.0, 0.0)
    assert tr.fill_small_regions(m) is m
    H, W = 75, 131
    out = torch.empty(3, 1, H, W, dtype=torch.float32, device="cuda")
    _lib.check(lib.cvmi_bilinear_f32(m.data_ptr(), 3, 96, 96, out.data_ptr(), H, W, None, 0.0, torch.cuda.current_stream().cuda_stream), "bilinear")
    assert torch.equal(tr.postprocess_masks(m, (H, W)), out)
    u8, ext = torch.empty(3, 1, H, W, dtype=torch.uint8, device="cuda"), torch.empty(3, 4, dtype=torch.int32, device="cuda")
    _lib.check(lib.cvmi_mask_postprocess(m.data_ptr(), 3, 96, 96, H, W, 0.0, u8.data_ptr(), ext.data_ptr(), torch.cuda.current_stream().cuda_stream), "pp")
    got_u8, got_boxes = tr.postprocess_to_mask(m, (H, W))
    assert torch.equal(got_u8, u8) and got_boxes == tr.extents_to_boxes(ext)
    sizes = [(75, 131), (96, 96), (40, 33)]
    sz = np.asarray(sizes, dtype=np.int32)
    packed, ext2 = torch.empty(int((sz[:, 0] * sz[:, 1]).sum()), dtype=torch.uint8, device="cuda"), torch.empty(3, 4, dtype=torch.int32, device="cuda")
    _lib.check(lib.cvmi_mask_postprocess_sizes(m.data_ptr(), 3, 96, 96, sz.ctypes.data, 0.0, packed.data_ptr(), ext2.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "pp_sizes")
    got, got_ext = tr.postprocess_to_masks_sized(m, sizes)
    assert torch.equal(torch.cat([g.reshape(-1) for g in got]), packed) and torch.equal(got_ext, ext2)


def test_composition_with_the_resize():
    """areas 8 / 8 then the resize == the resize (areas 0) of the reference's filled logits"""
    rng = np.random.RandomState(9)
    x = _logits(rng.rand(3, 96, 96) < 0.5, 0.0, 13)
    assert not np.array_equal(ref.fill_small(x, 0.0, 8, 8), x)
    dev, filled = torch.from_numpy(x)[:, None].cuda(), torch.from_numpy(ref.fill_small(x, 0.0, 8, 8))[:, None].cuda()
    tr8, tr0 = SAM2Transforms(96, 0.0, 8, 8), SAM2Transforms(96, 0.0, 0, 0)
    u8, boxes = tr8.postprocess_to_mask(dev, (75, 131))
    ru8, rboxes = tr0.postprocess_to_mask(filled, (75, 131))
    assert torch.equal(u8, ru8) and boxes == rboxes
    assert not torch.equal(u8, tr0.postprocess_to_mask(dev, (75, 131))[0])
    assert torch.equal(tr8.postprocess_masks(dev, (75, 131)), tr0.postprocess_masks(filled, (75, 131)))
    sizes = [(75, 131), (96, 96), (40, 33)]
    got, ext = tr8.postprocess_to_masks_sized(dev, sizes)
    want, rext = tr0.postprocess_to_masks_sized(filled, sizes)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.equal(ext, rext)


def test_determinism_and_side_stream():
    rng = np.random.RandomState(21)
    m = torch.from_numpy(rng.rand(3, 1, 200, 328) < 0.5).cuda()
    l1, c1 = get_connected_components(m)
    l2, c2 = get_connected_components(m)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        l3, c3 = get_connected_components(m)
    side.synchronize()
    assert torch.equal(l1, l2) and torch.equal(c1, c2) and torch.equal(l1, l3) and torch.equal(c1, c3)


SEG_SEED = 8                   # synthetic segmenter weights whose logits have small holes / sprinkles on the test images (asserted below)


def test_pipeline_filters_before_the_resize(tmp_path):
    """CircuitPipeline with SAM2Transforms(R, 0, 8, 8): image for image the masks of the same run's high_res logits taken through the reference
    fill and the areas-0 post-process -- the plain path and crop=True, device_glue=True."""
    from circuitvision_amd.pipeline import CircuitPipeline
    from circuitvision_amd.sam2 import SamSyntheticParams
    from circuitvision_amd.sam2_infer import SAM2Model
    from test_crop_gpu import NAMES
    from test_oracle_sam2_cpu import MINI, mini_targets
    from test_pipeline_gpu import _mini_setup
    images, det, _yo, seg, tr0, _so, R = _mini_setup(tmp_path, n_images=3)
    if SEG_SEED != 8:
        seg = SAM2Model(MINI, R, dtype="f32", use_refinement=True).load_params(SamSyntheticParams(seed=SEG_SEED, lora_targets=mini_targets(), std=0.05))
    tr8 = SAM2Transforms(R, 0, 8, 8)
    differ = 0
    for kw in ({}, {"crop": True, "crop_padding": 20, "device_glue": True}):
        if kw:
            det.names = det.model.names = dict(NAMES)                        # a label map with text / junction classes: real crop windows
        res = CircuitPipeline(det, seg, tr8, **kw).run_batch(images, "learned")
        torch.cuda.synchronize()
        hi = seg.plan(len(images), slot=0).high_res.view(len(images), 1, R, R).clone()          # one chunk: the logits of this run
        filled = torch.from_numpy(ref.fill_small(hi[:, 0].cpu().numpy(), 0.0, 8, 8))[:, None].cuda()
        assert len(res) == len(images)
        for b, (i, r) in enumerate(res):
            assert i == b
            want, boxes = tr0.postprocess_to_mask(filled[b:b + 1], tuple(r["image"].shape[:2]))
            assert r["mask"].shape == tuple(r["image"].shape[:2])
            assert torch.equal(r["mask"], want[0, 0]) and r["extent"] == boxes[0], (kw, b)
            differ += int(not torch.equal(want, tr0.postprocess_to_mask(hi[b:b + 1], tuple(r["image"].shape[:2]))[0]))
    assert differ > 0, "the filter changed no mask: the test would pass with the filter skipped"
