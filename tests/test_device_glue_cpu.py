"""Host side of the device-resident glue (circuitvision_amd/glue.py, csrc/glue_ops.hip): the entry points are declared and bound, the class-flag
table, the info record's decoder (proven here, without a GPU: every crop.json case's crop_debug_info survives encode -> decode unchanged),
and what `CircuitPipeline(device_glue=True)` refuses."""
import json
import os
import re

import numpy as np
import pytest

from circuitvision_amd import _lib, glue
from circuitvision_amd import crop as pcrop
from circuitvision_amd.pipeline import CircuitPipeline

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "crop.json")))["cases"]
ENTRY_POINTS = ("cvmi_stage2_crop", "cvmi_sam2_transform_rects_dev", "cvmi_mask_postprocess_rects_dev")


def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cvmi355.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    # the binding's argument count equals the declaration's
    for name in ENTRY_POINTS:
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    # the constants glue.py mirrors
    assert int(re.search(r"#define CVMI_GLUE_MAX_DET (\d+)", header).group(1)) == glue.MAX_DET >= 300
    assert int(re.search(r"#define CVMI_GLUE_INFO_HEAD (\d+)", header).group(1)) == glue.INFO_HEAD
    enum = re.search(r"enum \{\s*CVMI_GLUE_REASON = 0,.*?\};", header, re.S).group(0)
    words = {m.group(1): int(m.group(2)) for m in re.finditer(r"CVMI_GLUE_(\w+) = (\d+)", enum)}
    for nm in ("REASON", "DECISION", "APPLIED", "LINK", "CLUSTERS", "MAIN_SIZE", "MAIN_TEXT", "MAIN_ID", "MAIN_FIRST", "TOTAL", "COMPONENT_TYPE",
               "TEXT_TYPE", "PADDING", "BASIS_SET", "PADDED_SET", "FINAL_SET", "BASIS", "PADDED", "FINAL"):
        assert words[nm] == getattr(glue, "I_" + nm), nm
    assert max(words.values()) + 4 <= glue.INFO_HEAD


# the reference's label map (its classes.json: {name: id}, recorded as a fixture)
REFERENCE_CLASSES = {i: nm for nm, i in json.load(open(os.path.join(HERE, "golden", "classes.json"))).items()}


def test_class_flags_on_the_reference_class_list():
    fl = glue.class_flags(REFERENCE_CLASSES)
    assert fl.dtype == np.uint8 and fl.shape == (62,)
    by = {REFERENCE_CLASSES[i]: v for i, v in enumerate(fl.tolist())}
    NC, J, T, N = glue.FLAG_NOT_CLUSTERED, glue.FLAG_JUNCTION, glue.FLAG_TEXT, glue.FLAG_NON_COMPONENT
    assert by["text"] == NC | T | N and by["junction"] == J | N and by["crossover"] == NC | N and by["vss"] == NC | N and by["explanatory"] == NC | N
    assert sorted(k for k, v in by.items() if v) == ["crossover", "explanatory", "junction", "text", "vss"]
    assert glue.class_flags(["circuit", "resistor"]).tolist() == [NC | N, 0]               # (a list: ids are positions)
    # a {id: name} map with gaps, as ultralytics' names
    fl = glue.class_flags({0: "resistor", 3: "text"})
    assert fl.tolist() == [0, 0, 0, NC | T | N]
    assert glue.class_flags({}).shape == (0,)


@pytest.mark.parametrize("case", GOLD, ids=[c["name"] for c in GOLD])
def test_info_record_round_trip(case):
    """crop_debug_info -> the kernel's record -> crop_debug_info: unchanged, for every reference vector (float coordinates included: the
    basis box travels as four f64)."""
    win, info = pcrop.crop_window(case["boxes"], (case["height"], case["width"]), case["padding"])
    rec = glue.encode_info(info, case["boxes"])
    assert rec.dtype == np.int32 and rec.shape == (glue.INFO_HEAD + len(case["boxes"]),)
    back = glue.decode_info(rec, case["boxes"], (case["height"], case["width"]))
    assert set(back) == set(info)
    for k in info:
        assert back[k] == info[k] and type(back[k]) is type(info[k]), k
    e = case["expected"]
    assert back["crop_applied"] == e["crop_applied"] and [t["uid"] for t in back["text_bboxes_that_expanded_crop"]] == e["text_uids_that_expanded_crop"]
    assert (back["main_cluster_info"] or {}).get("example_uid") == e["main_cluster_example_uid"]


def test_decoder_covers_every_reason_and_decision():
    seen_r, seen_d = set(), set()
    for case in GOLD:
        _, info = pcrop.crop_window(case["boxes"], (case["height"], case["width"]), case["padding"])
        seen_r.add(info["reason_for_no_crop"])
        seen_d.add(info["crop_decision_source"])
    assert seen_r == set(glue.REASONS) and seen_d | {"unknown"} == set(glue.DECISIONS)


class _Duck:
    image_size = 64
    names = {0: "resistor"}

    def predict(self, images, verbose=False):
        raise AssertionError("not reached")


def test_device_glue_refuses_what_it_cannot_serve():
    d = _Duck()
    with pytest.raises(ValueError, match="device_glue"):
        CircuitPipeline(d, d, d, crop=True, device_glue=True)                              # duck-typed models
    with pytest.raises(ValueError, match="device_glue"):
        CircuitPipeline(d, d, d, crop=True, crop_fn=lambda im, bb: (im, bb, None), device_glue=True)
    with pytest.raises(ValueError, match="device_glue"):
        CircuitPipeline(d, d, d, crop=False, device_glue=True)
    assert CircuitPipeline(d, d, d, crop=True).device_glue is False                        # the default
