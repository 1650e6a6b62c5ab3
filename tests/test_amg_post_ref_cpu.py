"""Mask RLE and small-region removal without a GPU: the numpy / scipy reference the GPU tests compare with (tests/amg_post_ref.py) against
answers worked out by hand, a proof that the rows of tests/test_amg_post_gpu.py tell every deliberately wrong variant from the reference,
the preconditions those rows rely on, and the host side of the feature (declarations, bindings, the host utilities, the per-call arguments)."""
import os
import re
import types

import numpy as np
import pytest
import torch

import amg_post_ref as ref
from circuitvision_amd import _lib, amg_utils
from mask_cc_ref import label_plane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cvmi_mask_rle_workspace", "cvmi_mask_rle", "cvmi_mask_remove_small_workspace", "cvmi_mask_remove_small")


# ---- known answers ------------------------------------------------------------------------------------------------------------------------------
def test_rle_known_answers():
    assert ref.mask_to_rle(np.array([[0, 1], [1, 1]]))["counts"] == [1, 3]
    assert ref.mask_to_rle(np.array([[1, 0], [0, 0]]))["counts"] == [0, 1, 3]
    assert ref.mask_to_rle(np.zeros((3, 4)))["counts"] == [12] and ref.mask_to_rle(np.ones((5, 3)))["counts"] == [0, 15]
    assert ref.mask_to_rle(np.array([[0, 0, 1], [1, 0, 0]])) == {"size": [2, 3], "counts": [1, 1, 2, 1, 1]}      # column-major: 0 1 | 0 0 | 1 0
    pairs = dict(ref.rle_rows())["column_pairs"]
    assert ref.mask_to_rle(pairs[0])["counts"] == [14, 2, 14] and ref.mask_to_rle(pairs[1])["counts"] == [14, 1, 15]     # one run across the column end
    rows = dict(ref.rle_rows())
    assert ref.mask_to_rle(rows["alternating_clear_first"][0])["counts"] == [1] * 64                 # H * W runs
    assert ref.mask_to_rle(rows["alternating_set_first"][0])["counts"] == [0] + [1] * 64             # H * W + 1
    # a true checkerboard of even height joins its runs across every column end
    assert ref.mask_to_rle(rows["checker_clear_first"][0])["counts"] == [1] * 7 + ([2] + [1] * 6) * 7 + [1]
    assert len(ref.mask_to_rle(rows["checker_set_first"][0])["counts"]) == 58
    assert ref.area_from_rle({"size": [2, 3], "counts": [1, 1, 2, 1, 1]}) == 2


def test_removal_known_answers():
    out, info = ref.remove_small_regions(ref.art("#.#"), 2, "both")
    assert out.tolist() == [[255, 255, 255]] and info.tolist() == [1, 3, 0, 0, 2, 0, 1, 0]
    assert ref.remove_small_regions(ref.art("#.#"), 2, "both", "single_pass")[0].tolist() == [[0, 0, 0]]
    out, info = ref.remove_small_regions(np.zeros((1, 1), np.uint8), 2, "both")
    assert out.tolist() == [[255]] and info[0] == 1 and info[6] == 1
    out, info = ref.remove_small_regions(ref.art("#.#"), 2, "islands")                   # both small: the raster-first one stays
    assert out.tolist() == [[255, 0, 0]] and info.tolist() == [1, 1, 0, 0, 0, 0, 0, 1]
    out, info = ref.remove_small_regions(ref.art("1..", "...", "..."), 2, "islands")     # a lone small component stays as it is: no pixel changes
    assert out.tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0]] and info[0] == 0
    out, info = ref.remove_small_regions(ref.art("111", "1.1", "111"), 2, "holes")       # the fill writes 255, the other bytes stay 1
    assert out.tolist() == [[1, 1, 1], [1, 255, 1], [1, 1, 1]] and info.tolist() == [1, 9, 0, 0, 2, 2, 1, 0]
    out, info = ref.remove_small_regions(np.zeros((2, 3), np.uint8), 7, "islands")
    assert not out.any() and info.tolist() == [0, 0, 0, 0, 0, 0, 0, 0]                    # the empty plane's box


def test_exact_area_row_is_strict():
    rows = {r[0]: r for r in ref.remove_rows()}
    _, planes, a = rows["exact_areas"]
    out, info = ref.remove_small_stack(planes, a, 3)
    assert a == 4 and info[0, 6] == 3 and info[0, 7] == 6                                # the hole and the two islands of 3 go, those of 4 stay
    assert out[0, 0, :4].all() and not out[0, 5, 2:6].any() and out[0, 5, 9:12].all() and not out[0, 2, 1:4].any()
    assert not out[0, 0:2, 12:].any()                                                     # (3 pixels: ##, #. -- one 8-connected island)


def test_diagonal_rows():
    rows = {r[0]: r for r in ref.remove_rows()}
    _, planes, a = rows["diagonals"]
    for phases in (1, 2, 3):
        out, info = ref.remove_small_stack(planes, a, phases)
        assert np.array_equal(out, planes) and not info[:, 0].any()
    assert np.unique(label_plane(planes[0] != 0)[0]).tolist() == [0, 1]                  # the diagonal: one component
    assert ref.remove_small_stack(planes, a, 2, "islands_4_connected")[1][0, 7] == 4      # five single pixels, the first stays
    assert ref.remove_small_stack(planes, a, 1, "holes_4_connected")[1][1, 6] == 2        # the pocket would be a hole of its own


def test_keep_largest_rows_and_the_tie():
    rows = {r[0]: r for r in ref.remove_rows()}
    _, planes, a = rows["all_small"]
    out, info = ref.remove_small_stack(planes, a, 3)
    assert info[:, 1].tolist() == [3, 3] and info[:, 7].tolist() == [3, 5] and info[:, 0].tolist() == [1, 1]
    assert out[0, 2, 3:6].all() and out[1, 1, 1:4].all()                                  # plane 1: the raster-first of the two 3-pixel components
    lab, area = label_plane(planes[1] != 0)
    sizes = sorted(int(area[lab == l][0]) for l in np.unique(lab[lab > 0]))
    assert sizes == [2, 3, 3], "the tie row has no size tie"
    assert ref.remove_small_stack(planes, a, 3, "keep_last_largest")[0][1, 3:5, 5:7].any()


# ---- round trip, mutants, preconditions ---------------------------------------------------------------------------------------------------------------
def test_rle_round_trip_on_every_row():
    for rid, planes in ref.rle_rows():
        offsets, counts = ref.stack_rle(planes)
        assert offsets[-1] == counts.size
        for n, p in enumerate(planes):
            rle = ref.mask_to_rle(p)
            assert rle["counts"] == counts[offsets[n]:offsets[n + 1]].tolist()
            assert sum(rle["counts"]) == p.size and rle["size"] == list(p.shape), rid
            assert np.array_equal(ref.rle_to_mask(rle), p != 0), rid
            assert np.array_equal(amg_utils.rle_to_mask(rle), p != 0) and amg_utils.rle_to_mask(rle).dtype == np.bool_, rid
            assert ref.area_from_rle(rle) == amg_utils.area_from_rle(rle) == int((p != 0).sum()), rid


def test_rle_rows_cover_what_the_issue_lists():
    rows = dict(ref.rle_rows())
    assert {(m.shape[1], m.shape[2]) for m in rows.values()} >= {(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (8, 8), (63, 65), (64, 64), (65, 63), (130, 70), (1, 300), (300, 1), (9, 9)}
    m = rows["planes_33"]
    assert m.shape[0] == 33 and not m[0].any() and not m[32].any() and m[1].all() and m[8].all()
    for rid in ("random_130x70_d0.5", "random_130x70_d0.02"):
        assert 0 < (rows[rid] != 0).mean() < 1


def test_the_rows_tell_every_mutant_from_the_reference():
    for mutant in ref.RLE_MUTANTS:
        hits = [rid for rid, planes in ref.rle_rows() if any(ref.mask_to_rle(p, mutant) != ref.mask_to_rle(p) for p in planes)]
        assert hits, mutant
    for mutant in ref.REMOVE_MUTANTS:
        hits = [rid for rid, planes, a in ref.remove_rows() if any(not np.array_equal(ref.remove_small_stack(planes, a, ph, mutant)[0], ref.remove_small_stack(planes, a, ph)[0])
                                                                    for ph in (1, 2, 3))]
        assert hits, mutant
    dicts, a, t = ref.post_case()
    want = ref.postprocess_small_regions(list(dicts), a, t)
    for mutant in ref.POST_MUTANTS:
        got = ref.postprocess_small_regions(list(dicts), a, t, mutant=mutant)
        assert [(d["predicted_iou"], d["bbox"]) for d in got] != [(d["predicted_iou"], d["bbox"]) for d in want], mutant


def test_preconditions_of_the_gpu_rows():
    rows = {r[0]: r for r in ref.remove_rows()}
    for rid in ref.SEEDED_REMOVE_ROWS + ("spiral_130",):
        _, planes, a = rows[rid]
        for phases in ((2, 3) if rid == "spiral_130" else (1, 2, 3)):
            changed = ref.remove_small_stack(planes, a, phases)[1][:, 0]
            assert changed.any() and not changed.all(), (rid, phases)
    assert rows["blobs_33_planes"][1].shape[0] == 33 and rows["blobs_130x70"][1].shape[1:] == (130, 70)
    _, planes, a = rows["plain"]
    assert not planes[0].any() and (planes[1] == 255).all() and set(np.unique(planes[2]).tolist()) == {0, 1}
    assert np.array_equal(ref.remove_small_stack(planes, a, 3)[0], planes)
    for rid in ("blobs_63x65", "blobs_130x70"):                                          # components and holes ON the 64-pixel seams
        _, planes, a = rows[rid]
        fg = planes[1:] != 0
        assert (fg[:, :, 63] & fg[:, :, 64]).any() and not (fg[:, :, 63] & fg[:, :, 64]).all()         # foreground and background across the column seam
        assert planes.shape[1] < 65 or (fg[:, 63] & fg[:, 64]).any()                                   # ... and across the row seam
    dicts, a, t = ref.post_case()
    out = ref.postprocess_small_regions(list(dicts), a, t)
    assert [d["predicted_iou"] for d in out] == [0.85, 0.8, 0.9], "unchanged first (2, 3), then the changed 0; 1 suppressed by 2"
    assert len(out) < len(dicts), "no second-NMS suppression"
    assert out[2]["bbox"] != dicts[0]["bbox"] and out[2]["area"] == dicts[0]["area"] - 1
    assert all(d["area"] == int((d["segmentation"] != 0).sum()) for d in out)
    rle = ref.postprocess_small_regions(list(dicts), a, t, output_mode="uncompressed_rle")
    assert all(np.array_equal(ref.rle_to_mask(r["segmentation"]), o["segmentation"].numpy() != 0) and r["area"] == ref.area_from_rle(r["segmentation"])
               for r, o in zip(rle, out))


# ---- the host side --------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cvmi355.h")).read()
    for name in ENTRY_POINTS:
        decl = re.search(r"\n(?:size_t|int) %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert name in _lib.SIGNATURES, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "mask_rle.o" in open(os.path.join(ROOT, "circuitvision_amd", "csrc", "Makefile")).read()
    assert amg_utils.REMOVE_SMALL_WORKSPACE_BYTES == 1 << 30 and amg_utils.REMOVE_SMALL_WORKSPACE_BYTES // (8 * 1024 * 1024) == 128
    assert amg_utils.PHASES == {"holes": 1, "islands": 2, "both": 3} and amg_utils.INFO == ref.INFO


def test_host_utilities_refuse_bad_input():
    with pytest.raises(ValueError):
        amg_utils.rle_to_mask({"size": [2, 2], "counts": [3]})
    with pytest.raises(ValueError):
        amg_utils.mask_to_rle(torch.zeros(2, 3, 3, dtype=torch.uint8))                   # not on the device
    with pytest.raises(ValueError):
        amg_utils.remove_small_regions(torch.zeros(2, 3, 3, dtype=torch.uint8), 4, "everything")
    assert amg_utils.postprocess_small_regions([], 4, 0.7) == []


def test_per_call_arguments_and_the_constructor_messages():
    import inspect
    from circuitvision_amd.amg import Sam2AutomaticMaskGenerator
    model = types.SimpleNamespace(image_size=256)
    for kw, word in ((dict(min_mask_region_area=10), "generate(image, min_mask_region_area"), (dict(output_mode="uncompressed_rle"), "generate(image, output_mode"),
                     (dict(output_mode="coco_rle"), "per-call")):
        with pytest.raises(NotImplementedError, match=re.escape(word)):
            Sam2AutomaticMaskGenerator(model, **kw)
    gen = Sam2AutomaticMaskGenerator(model, points_per_side=2)
    for fn in (gen.generate, gen.generate_batch):
        p = inspect.signature(fn).parameters
        assert p["min_mask_region_area"].default == 0 and p["output_mode"].default == "binary_mask"
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    with pytest.raises(NotImplementedError, match="pycocotools"):
        gen.generate(img, output_mode="coco_rle")
    with pytest.raises(ValueError, match="output_mode"):
        gen.generate_batch([], output_mode="polygons")
    with pytest.raises(ValueError, match="min_mask_region_area"):
        gen.generate_batch([], min_mask_region_area=-1)
