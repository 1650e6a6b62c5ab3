"""Generate tests/golden/terminal_reclass.json from the reference's OWN CircuitAnalyzer.reclassify_terminals_based_on_connectivity and
segment_circuit (build container only).

Both methods are called unbound on a carrier object that holds `debug = False`, a `yolo.model.names` dict and the helper methods the first
calls on self (segment_circuit, get_contours, is_point_near_bbox), taken unbound from the same class.  The reference's modules are imported
behind the stub modules of make_golden.py; OpenCV is not installed, so a stand-in `cv2` answers the calls the methods make with THE
PROJECT'S restatements: make_node_golden.py's stand-in (mean / findContours / contourArea / boundingRect / moments from tests/wire_ref.py and
tests/node_ref.py, drawings that draw nothing) plus cvtColor (RGB2BGR: the channels reversed; RGB2GRAY: segment_ref.grey with the R weight
on channel 0) and adaptiveThreshold (segment_ref.adaptive_threshold, which refuses any other arguments than the reference's).

WHAT THIS PINS: the reference's control flow over our OpenCV restatement -- the order of the two channel swaps, the emptying slices (no
ymin < ymax guard, so a negative xmax counts from the end), get_contours' area threshold 0.0001, the point test with threshold 10 and no
broad phase, the `>= 2` rule and the keys it writes.  It does NOT pin OpenCV's arithmetic: a mistake in the restated grey conversion, box
mean, threshold or contours would be in both sides of the comparison.

The fixture is DATA: inputs as generator seeds (segment_ref.golden_image) plus the box dicts and the names; outputs as the box dicts after
the call, the call's return value, and the shape, sum and a checksum of segment_circuit's mask of the same image.  No reference source text is
stored.
Usage:  python tests/golden/make_terminal_golden.py   (needs the reference checkout; never runs on the GPU box)
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import make_golden as MG  # noqa: E402
import make_node_golden as MN  # noqa: E402
import segment_ref as S  # noqa: E402

NAMES = {0: "resistor", 1: "terminal", 2: "voltage.dc", 3: "junction", 4: "text"}
NAMES_WITHOUT_DC = {0: "resistor", 1: "terminal", 3: "junction"}


def stand_in_cv2():
    cv = MN.stand_in_cv2([])
    cv.COLOR_RGB2BGR, cv.COLOR_RGB2GRAY, cv.ADAPTIVE_THRESH_MEAN_C, cv.THRESH_BINARY_INV = 4, 7, 0, 1

    def cvt(img, code):
        if code == cv.COLOR_RGB2BGR:
            return np.ascontiguousarray(img[..., ::-1])
        if code == cv.COLOR_RGB2GRAY:
            return S.grey(img, 0)
        return 1 / 0
    cv.cvtColor = cvt
    cv.adaptiveThreshold = lambda img, mx, method, kind, k, c: S.adaptive_threshold(img, k, c) if (mx, method, kind, k, c) == (255, 0, 1, 31, 21) else 1 / 0
    return cv


def _b(cls, x0, y0, x1, y1, cid):
    return {"class": cls, "_yolo_class_id_temp": cid, "confidence": 0.5, "xmin": x0, "ymin": y0, "xmax": x1, "ymax": y1,
            "persistent_uid": f"{cls}_{x0}_{y0}_{x1}_{y1}"}


H, WD = 200, 240
WIRES = [[100, 50, 200, 54], [140, 100, 215, 104], [180, 150, 230, 154]]      # three horizontal wires [x0, y0, x1, y1) with staggered ends
EDGE_ONLY = (55, 130, 98, 140)        # overlaps no wire: its xmax LINE passes 2 px from wire 0's left end, its ymax LINE 10 px above wire 2


def cases():
    """(name, image spec, names, boxes, connected contours per terminal as segment_ref counts them)."""
    def spec(wires=WIRES, seed=1):
        return {"gen": "segments", "h": H, "w": WD, "seed": seed, "segments": wires}

    def term(x0, y0, x1, y1):
        return _b("terminal", x0, y0, x1, y1, 1)
    out = []
    out.append(("terminal_on_0_1_2_3_wires", spec(), NAMES, [term(9, 13, 37, 81), term(226, 140, 238, 170), term(*EDGE_ONLY), term(170, 101, 205, 129)],
                [0, 1, 2, 3]))
    out.append(("edge_line_rule_without_overlap", spec(), NAMES, [term(*EDGE_ONLY)], [2]))
    out.append(("preserved_class_is_not_emptied", spec(), NAMES, [_b("junction", 90, 0, WD, H, 3), term(*EDGE_ONLY)], [2]))
    out.append(("emptied_resistor_cuts_a_wire_in_two", spec(WIRES[:1]), NAMES, [_b("resistor", 150, 40, 160, 60, 0), term(145, 20, 165, 35)], [2]))
    out.append(("uncut_wire_for_comparison", spec(WIRES[:1]), NAMES, [term(145, 20, 165, 35)], [0]))
    # a 2 x 2 speck 6 px under the terminal's ymax line: its contour has area 1 / 48000 of the plane, below get_contours' 0.0001
    out.append(("speck_below_the_area_threshold", spec([WIRES[0], [100, 66, 102, 68]]), NAMES, [term(90, 40, 110, 60)], [1]))
    out.append(("negative_xmax", spec(), NAMES, [_b("text", 20, 0, -30, H, 4), term(*EDGE_ONLY)], [1]))     # columns 20 .. W - 30 emptied: wire 0 is gone
    # a wire of colour (255, 230, 0): grey 164 with the R weight on channel 2 (the method's own swap), 211 with it on channel 0, on a page of
    # grey 235 / 228 -- only the reference's channel order puts it 21 below the mean
    out.append(("wire_seen_only_in_the_reference_channel_order", spec([WIRES[0], WIRES[2] + [255, 230, 0]]), NAMES, [term(*EDGE_ONLY)], [2]))
    out.append(("names_without_voltage_dc", spec(), NAMES_WITHOUT_DC, [term(*EDGE_ONLY)], [2]))
    out.append(("no_terminals", spec(), NAMES, [_b("resistor", 40, 40, 80, 120, 0), _b("junction", 100, 150, 106, 156, 3)], []))
    bb = [term(30, 40, 60, 70), term(120, 60, 150, 100), _b("resistor", 70, 20, 110, 50, 0), term(10, 90, 30, 110)]
    out.append(("synthetic_circuit", {"gen": "circuit", "h": 120, "w": 200, "seed": 2}, NAMES, bb, None))
    return out


def main():
    MG.import_reference()
    analyzer = MG.import_analyzer()
    mod = sys.modules[analyzer.__module__]
    mod.cv2 = stand_in_cv2()

    def run(spec, names, bboxes):
        carrier = types.SimpleNamespace(debug=False, yolo=types.SimpleNamespace(model=types.SimpleNamespace(names=dict(names))))
        for name in ("segment_circuit", "get_contours", "is_point_near_bbox"):
            setattr(carrier, name, types.MethodType(getattr(analyzer, name), carrier))
        image = S.golden_image(spec)
        after = [dict(b) for b in bboxes]
        ret = analyzer.reclassify_terminals_based_on_connectivity(carrier, image.copy(), after)
        mask = analyzer.segment_circuit(carrier, image.copy())
        return {"returns_none": ret is None, "bboxes": after, "segment_circuit": S.mask_summary(mask)}
    fixture = []
    for n, sp, names, bb, counts in cases():
        mine = [dict(b) for b in bb]
        got, _ = S.reclassify(S.golden_image(sp), mine, names, red_channel=2)
        assert counts is None or [got[k] for k in sorted(got)] == counts, (n, got)       # the cases are what their names say
        fixture.append({"name": n, "image": sp, "names": {str(k): v for k, v in names.items()}, "bboxes": bb, "expect": run(sp, names, bb)})
        assert fixture[-1]["expect"]["bboxes"] == mine, n                                 # the restatement follows the reference's control flow
        assert fixture[-1]["expect"]["returns_none"], n
        if n == "speck_below_the_area_threshold":
            assert S.reclassify(S.golden_image(sp), [dict(b) for b in bb], names, red_channel=2, area_threshold=-1.0)[0] == {0: 2}
        if n == "wire_seen_only_in_the_reference_channel_order":
            assert S.reclassify(S.golden_image(sp), [dict(b) for b in bb], names, red_channel=0)[0] == {0: 1}
    by = {c["name"]: c["expect"]["bboxes"] for c in fixture}
    done = by["terminal_on_0_1_2_3_wires"][2]
    assert [b["class"] for b in by["terminal_on_0_1_2_3_wires"]] == ["terminal", "terminal", "voltage.dc", "voltage.dc"]
    assert done["_yolo_class_id_temp"] == 2 and done["was_reclassified_from_terminal"] is True and done["original_yolo_class_if_reclassified"] == "terminal"
    assert by["names_without_voltage_dc"][0]["class"] == "voltage.dc" and by["names_without_voltage_dc"][0]["_yolo_class_id_temp"] == 1
    assert by["negative_xmax"][1]["class"] == "terminal" and by["no_terminals"] == [c for c in cases() if c[0] == "no_terminals"][0][3]
    path = os.path.join(HERE, "terminal_reclass.json")
    with open(path, "w") as f:
        json.dump({"what": "reference control flow of reclassify_terminals_based_on_connectivity / segment_circuit over the project's OpenCV "
                           "restatement (see make_terminal_golden.py)", "cases": fixture}, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes,", len(fixture), "cases")


if __name__ == "__main__":
    main()
