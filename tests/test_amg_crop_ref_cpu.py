"""The automatic mask generator's crop layers without a GPU: the crop geometry's known answers against both the reference (tests/amg_crop_ref.py)
and amg_utils, a proof that the rows of tests/test_amg_crop_gpu.py tell every deliberately wrong variant from the reference, and the host side of
the feature (declarations, bindings, the per-call arguments and their refusals)."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import amg_crop_ref as cref
import amg_ref
from circuitvision_amd import _lib, amg_utils
from test_amg_ref_cpu import _amg_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cvmi_amg_select_crop", "cvmi_amg_score_window")


def window_rows():
    return cref.WINDOW_ROWS + (cref.grid_cap_window_row(*_amg_constants()),)


# ---- known answers --------------------------------------------------------------------------------------------------------------------------------------
KNOWN = (
    ((1200, 1800), 1, {0: [0, 0, 1800, 1200], 1: [0, 0, 1105, 805], 2: [0, 396, 1105, 1200], 3: [696, 0, 1800, 805], 4: [696, 396, 1800, 1200]}, 5),
    ((96, 160), 1, {0: [0, 0, 160, 96], 1: [0, 0, 96, 64], 2: [0, 32, 96, 96], 3: [64, 0, 160, 64], 4: [64, 32, 160, 96]}, 5),
    ((61, 77), 1, {0: [0, 0, 77, 61], 1: [0, 0, 49, 41], 2: [0, 21, 49, 61], 3: [29, 0, 77, 41], 4: [29, 21, 77, 61]}, 5),
    ((256, 256), 2, {0: [0, 0, 256, 256], 1: [0, 0, 172, 172], 2: [0, 85, 172, 256], 3: [85, 0, 256, 172], 4: [85, 85, 256, 256], 5: [0, 0, 97, 97],
                     6: [0, 54, 97, 151], 7: [0, 108, 97, 205], 8: [0, 162, 97, 256], 20: [162, 162, 256, 256]}, 21),
    ((96, 160), 2, {5: [0, 0, 52, 36], 6: [0, 20, 52, 56], 7: [0, 40, 52, 76], 8: [0, 60, 52, 96], 20: [108, 60, 160, 96]}, 21),
)


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: "%dx%d_layers%d" % (c[0][0], c[0][1], c[1]))
def test_crop_boxes_known_answers(case):
    (H, W), layers, known, count = case
    for boxes, idxs in (cref.crop_boxes(H, W, layers), amg_utils.generate_crop_boxes((H, W), layers, 512 / 1500)):
        assert len(boxes) == len(idxs) == count
        assert all(list(boxes[i]) == b for i, b in known.items()), boxes
        assert list(idxs) == [0] + [1] * 4 + [2] * 16 * (layers - 1)
        assert all(0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H for x0, y0, x1, y1 in boxes)
    assert amg_utils.generate_crop_boxes((H, W), 0, 512 / 1500) == ([[0, 0, W, H]], [0])


def test_layer_grids_known_answers():
    for n, sides in ((32, (32, 16, 8)), (4, (4, 2, 1))):
        for grids in (cref.layer_grids(n, 2, 2), amg_utils.build_all_layer_point_grids(n, 2, 2)):
            assert [len(g) for g in grids] == [s * s for s in sides]
            for g, s in zip(grids, sides):
                assert np.array_equal(g, amg_ref.point_grid(s)) and g.dtype == np.float64
    assert np.array_equal(amg_utils.build_all_layer_point_grids(4, 2, 2)[2], [[0.5, 0.5]])
    assert [len(g) for g in amg_utils.build_all_layer_point_grids(5, 1, 1)] == [25, 25]
    with pytest.raises(ValueError, match="layer 3"):
        amg_utils.build_all_layer_point_grids(4, 3, 2)
    # the unequal layer-1 areas of the 256 x 256 image, which the NMS across the crops orders by
    b = cref.crop_boxes(256, 256, 1)[0]
    assert [(x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in b[1:]] == [172 * 172, 172 * 171, 171 * 172, 171 * 171]


def test_border_cases_are_what_their_labels_say():
    seen = set()
    for crop, (W, H), rows in cref.BORDER_CASES:
        boxes = [b for _, b, _ in rows]
        assert cref.near_crop_edge(boxes, crop, H, W).tolist() == [not kept for _, _, kept in rows], crop
        assert all(0 <= b[0] <= b[2] < crop[2] - crop[0] and 0 <= b[1] <= b[3] < crop[3] - crop[1] for b in boxes)
        seen |= {label for label, _, _ in rows}
        kept = [k for _, _, k in rows]
        assert any(not kept[i] and any(kept[:i]) and any(kept[i + 1:]) for i in range(len(kept)))       # a dropped candidate between two kept ones
    assert seen >= {s + d for s in ("left_", "top_", "right_", "bottom_") for d in ("20", "21")} | {"empty_at_the_origin", "empty_in_interior_crop", "both_edges"}
    assert [c for c, _, _ in cref.BORDER_CASES][:2] == [[64, 32, 160, 96], [85, 85, 256, 256]]


# ---- the rows tell every mutant from the reference --------------------------------------------------------------------------------------------------------
def _merge(mutant=None, info=None):
    crops, H, W, t = cref.merge_case()
    return cref.generate_crops_ref(crops, H, W, mutant=mutant, info=info, **t)


def test_the_merge_case_exercises_every_stage():
    info = {}
    out = _merge(info=info)
    per = info["per_crop"]
    assert any(p["cut"] > 0 and p["passed"] - p["cut"] > 0 for p in per[1:]), per                    # the border filter drops and keeps in one interior crop
    assert per[0]["cut"] == 0
    assert sum(p["suppressed"] for p in per) > 0 and info["cross_suppressed"] > 0, info
    assert 0 in info["crops_in_result"] and len([c for c in info["crops_in_result"] if c > 0]) >= 2, info
    assert all(tuple(d) == amg_ref.KEYS and tuple(d["segmentation"].shape) == (256, 256) for d in out)
    assert all(d["area"] == int((d["segmentation"] != 0).sum()) for d in out)
    for d in out:                                                                # box, point and mask agree in image coordinates
        ys, xs = torch.nonzero(d["segmentation"], as_tuple=True)
        assert d["bbox"] == [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]
        cx0, cy0, cw, ch = d["crop_box"]
        assert cx0 <= d["point_coords"][0][0] < cx0 + cw and cy0 <= d["point_coords"][0][1] < cy0 + ch
    areas = [d["crop_box"][2] * d["crop_box"][3] for d in out]
    assert areas == sorted(areas) and len(set(areas)) >= 3                                           # smaller crops first; the unequal layer-1 areas take part
    assert amg_ref.same_dicts(out, _merge())


def test_the_rows_tell_every_mutant_from_the_reference():
    want = _merge()
    for mutant in cref.CROP_MUTANTS:
        hits = []
        if mutant in ("tol_lt", "box_max_exclusive", "image_edge_not_exempt"):
            hits = [crop for crop, (W, H), rows in cref.BORDER_CASES
                    if cref.near_crop_edge([b for _, b, _ in rows], crop, H, W, mutant=mutant).tolist() != [not k for _, _, k in rows]]
        elif mutant in ("crop_order_yx", "overlap_ceil"):
            hits = [hw for hw in ((256, 256), (96, 160)) if cref.crop_boxes(*hw, 2, mutant=mutant) != cref.crop_boxes(*hw, 2)]
        elif mutant == "grid_not_downscaled":
            hits = [n for n in (4,) if [len(g) for g in cref.layer_grids(n, 2, 2, mutant)] != [len(g) for g in cref.layer_grids(n, 2, 2)]]
        elif mutant == "window_off_by_one":
            for row in window_rows():
                H, W, PH, PW, wx0, wy0 = row[4:]
                mask = (torch.rand(H, W, generator=torch.Generator().manual_seed(H + W)) > 0.5).to(torch.uint8) * 255
                crop = [wx0, wy0, wx0 + W, wy0 + H]
                if not torch.equal(cref.uncrop_mask(mask, crop, PH, PW, mutant), cref.uncrop_mask(mask, crop, PH, PW)):
                    hits.append(row[0])
            assert not amg_ref.same_dicts(_merge(mutant), want), mutant
        else:
            hits = [mutant] if not amg_ref.same_dicts(_merge(mutant), want) else []
        assert hits, mutant


def test_window_rows_cover_what_the_issue_lists():
    rows = {r[0]: r for r in window_rows()}
    cap, chunk = _amg_constants()
    for r in rows.values():
        M, h, w, H, W, PH, PW, wx0, wy0 = r[1:]
        assert 0 <= wx0 and wx0 + W <= PW and 0 <= wy0 and wy0 + H <= PH and M > 0, r[0]
    assert {(r[8], r[9]) for r in rows.values() if (r[4], r[5], r[6], r[7]) == (33, 45, 64, 64)} == {(x, y) for x in (0, 1, 2, 3, 19) for y in (0, 31)}
    assert 19 + 45 == 64 and 31 + 33 == 64                                                          # right-flush, bottom-flush
    assert {r[7] for r in rows.values()} >= {63, 66} and rows["pw63_bytes_odd_stride"][1] == 3 and (35 * 63) % 2 == 1
    assert rows["one_pixel_plane"][4:8] == (1, 1, 1, 1) and rows["one_pixel_in_5x7"][4:8] == (1, 1, 5, 7)
    assert rows["window_is_plane_64x64"][4:8] == (64, 64, 64, 64) and rows["window_is_plane_67x131"][4:8] == (67, 131, 67, 131)
    assert rows["past_one_chunk_1x1028"][6:9] == (1, 1028, 1024) and rows["past_one_chunk_1x1028"][5] == 4 and chunk == 1024
    g = rows["grid_cap_plus_1"]
    assert -(-g[7] // chunk) > cap and g[6] == 1 and g[8] < cap * chunk < g[8] + g[5]               # more units than the cap; the window crosses into the last one


# ---- the host side ----------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cvmi355.h")).read()
    for name in ENTRY_POINTS:
        decl = re.search(r"\nint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert name in _lib.SIGNATURES, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert len(_lib.SIGNATURES["cvmi_amg_select_crop"][1]) == len(_lib.SIGNATURES["cvmi_amg_select"][1]) + 7
    assert len(_lib.SIGNATURES["cvmi_amg_score_window"][1]) == len(_lib.SIGNATURES["cvmi_amg_score"][1]) + 4


def test_per_call_arguments_and_the_refusals():
    from circuitvision_amd import amg
    model = types.SimpleNamespace(image_size=256)
    with pytest.raises(NotImplementedError, match=re.escape("generate(image, crop_n_layers")):
        amg.Sam2AutomaticMaskGenerator(model, crop_n_layers=1)
    with pytest.raises(NotImplementedError, match="use_m2m"):
        amg.Sam2AutomaticMaskGenerator(model, use_m2m=True)
    gen = amg.Sam2AutomaticMaskGenerator(model, points_per_side=2)
    for fn in (gen.generate, gen.generate_batch):
        p = inspect.signature(fn).parameters
        assert p["crop_n_layers"].default == 0 and p["crop_overlap_ratio"].default == 512 / 1500
        assert p["crop_n_points_downscale_factor"].default == 1 and p["crop_nms_thresh"].default == 0.7
        assert p["min_mask_region_area"].default == 0 and p["output_mode"].default == "binary_mask"
    assert amg.CROP_EDGE_TOL == cref.EDGE_TOL == 20 and amg.build_point_grid is amg_utils.build_point_grid
    with pytest.raises(ValueError, match="list of RGB u8 images"):
        gen.generate_batch(torch.zeros(1, 3, 256, 256), orig_hw=[(8, 8)], crop_n_layers=1)
    with pytest.raises(ValueError, match="crop_n_layers"):
        gen.generate_batch([], crop_n_layers=-1)
    with pytest.raises(ValueError, match="layer 2"):                                                # 2 points per side, downscaled twice by 2: no point left
        gen.generate_batch([np.zeros((8, 8, 3), np.uint8)], crop_n_layers=2, crop_n_points_downscale_factor=2)
    assert gen.generate_batch([], crop_n_layers=1) == []
    explicit = amg.Sam2AutomaticMaskGenerator(model, points_per_side=None, point_grids=[amg_ref.point_grid(2)])
    with pytest.raises(ValueError, match="points_per_side"):
        explicit.generate(np.zeros((8, 8, 3), np.uint8), crop_n_layers=1)
    with pytest.raises(ValueError, match="output_mode"):
        gen.generate_batch([], output_mode="polygons", crop_n_layers=1)
