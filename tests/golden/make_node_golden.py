"""Generate tests/golden/node_connections.json from the reference's OWN CircuitAnalyzer.get_node_connections (build container only).

The method is called unbound on a carrier object that holds only `debug`, `non_components` and `source_components` (plus the helper
methods it calls on self, taken unbound from the same class, and a show_image that shows nothing).  `debug` is True: with debug=False the
method raises UnboundLocalError at :1330 for any non-empty box list (`problematic_terminal_uid` is assigned only under `if self.debug:`,
:1311-1313), so debug=True is the only mode in which it returns; its debug branches print, draw and show, and change no result.
The reference's modules are imported behind the stub modules of make_golden.py; OpenCV is not installed, so a stand-in `cv2` answers the
calls the method makes with THE PROJECT'S restatements
(tests/wire_ref.py for resize / GaussianBlur / dilate / erode / mean / findContours / contourArea / boundingRect, tests/node_ref.py for
moments); cvtColor gives the grey plane three channels, and drawContours / putText / circle / rectangle draw nothing (circle notes its
centre: that is how the connection points, which the reference only draws, reach the fixture).

WHAT THIS PINS: the reference's control flow over our OpenCV restatement -- which boxes it visits, the broad phase, the point test and
its thresholds, the de-duplication, the ground choice and the renumbering.  It does NOT pin OpenCV's arithmetic: a mistake in the
restated contours or moments would be in both sides of the comparison.

The fixture is DATA: inputs as generator seeds (node_ref.golden_mask) plus the box dicts; outputs as, per node, its id, the components'
uids / classes / resized coordinates, the contour's point count and a checksum of its points, then the connection points and the shapes of
the five returned images.  No reference source text is stored.
Usage:  python tests/golden/make_node_golden.py   (needs the reference checkout; never runs on the GPU box)
"""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import make_golden as MG  # noqa: E402
import node_ref as R  # noqa: E402
import wire_ref as W  # noqa: E402
from oracle.preprocess import resize_linear_u8  # noqa: E402


def stand_in_cv2(circles):
    cv = types.ModuleType("cv2")
    cv.COLOR_GRAY2BGR, cv.RETR_EXTERNAL, cv.CHAIN_APPROX_SIMPLE, cv.FONT_HERSHEY_SIMPLEX = 8, 0, 2, 0
    cv.resize = lambda img, size: resize_linear_u8(img[..., None], size[0], size[1])[..., 0]
    cv.GaussianBlur = lambda img, k, s: W.gaussian_blur_5x5(img) if (tuple(k), s) == ((5, 5), 1) else 1 / 0
    cv.dilate = lambda img, kernel, iterations: W.dilate2(img) if (kernel.shape, iterations) == ((3, 3), 2) else 1 / 0
    cv.erode = lambda img, kernel, iterations: W.erode2(img) if (kernel.shape, iterations) == ((3, 3), 2) else 1 / 0
    cv.mean = lambda img: (int(img.astype(np.int64).sum()) / img.size, 0.0, 0.0, 0.0)
    cv.findContours = lambda img, mode, method: (tuple(np.array(p, dtype=np.int32).reshape(-1, 1, 2) for p in W.find_external_contours(img != 0)), None)
    cv.contourArea = lambda c: abs(W.shoelace2([tuple(int(v) for v in p) for p in c.reshape(-1, 2)])) / 2.0
    cv.boundingRect = lambda c: W.bounding_rect([tuple(int(v) for v in p) for p in c.reshape(-1, 2)])
    cv.moments = R.moments
    cv.cvtColor = lambda img, code: np.repeat(img[..., None], 3, axis=2)
    cv.drawContours = cv.putText = cv.rectangle = lambda img, *a, **k: img
    cv.circle = lambda img, centre, **k: circles.append([int(centre[0]), int(centre[1])]) or img
    return cv


def _b(cls, x0, y0, x1, y1, uid="auto", **extra):
    d = {"class": cls, "confidence": 0.5, "xmin": x0, "ymin": y0, "xmax": x1, "ymax": y1}
    if uid is not None:
        d["persistent_uid"] = f"{cls}_{x0}_{y0}_{x1}_{y1}" if uid == "auto" else uid
    d.update(extra)
    return d


def cases():
    H, Wd = 300, 200

    def spec(seed):
        return {"gen": "rails", "h": H, "w": Wd, "seed": seed}

    def between(seed, i, j, x, cls, uid="auto", wdt=20):             # a box from rail i down to rail j, one pixel into each
        rows, _ = R.rails(H, Wd, seed)
        return _b(cls, x, rows[i][1] - 1, x + wdt, rows[j][0] + 1, uid)

    def above(seed, i, x, cls, uid="auto"):                           # a box that ends one pixel into rail i
        rows, _ = R.rails(H, Wd, seed)
        return _b(cls, x, rows[i][0] - 30, x + 20, rows[i][0] + 1, uid)
    out = []
    out.append(("source_on_two_nodes", spec(1), [between(1, 0, 1, 40, "voltage.dc"), between(1, 0, 1, 120, "resistor"),
                                                 between(1, 1, 2, 60, "capacitor.unpolarized"), between(1, 1, 2, 140.6, "inductor"),
                                                 _b("text", 5, 5, 30, 15), _b("junction", 100, 150, 106, 156)]))
    out.append(("no_source_second_tier", spec(3), [between(3, 0, 1, 40, "resistor"), between(3, 0, 1, 90, "capacitor.unpolarized"),
                                                   between(3, 0, 1, 140, "diode")]))
    out.append(("two_valid_nodes_one_single", spec(6), [between(6, 0, 1, 60, "resistor"), above(6, 0, 120, "resistor")]))
    out.append(("three_valid_nodes_single_dropped", spec(4), [between(4, 0, 1, 50, "resistor"), between(4, 0, 1, 100, "capacitor.unpolarized"),
                                                              between(4, 1, 2, 150, "inductor")]))
    out.append(("box_without_uid", spec(0), [between(0, 0, 1, 50, "resistor", uid=None), between(0, 0, 1, 50, "resistor", uid=None),
                                             between(0, 0, 1, 120, "transistor.bjt")]))
    out.append(("two_boxes_share_a_uid", spec(2), [between(2, 0, 1, 40, "resistor", uid="dup"), between(2, 0, 1, 110, "capacitor.polarized", uid="dup"),
                                                   between(2, 1, 2, 150, "current.dc")]))
    rows5, (x0, x1) = R.rails(H, Wd, 5)
    out.append(("no_valid_node", spec(5), [_b("text", 50, rows5[0][0] - 3, 90, rows5[0][1] + 3), _b("junction", 100, rows5[1][0], 106, rows5[1][1]),
                                           _b("resistor", Wd - 12, 100, Wd - 2, 130)]))
    rng = np.random.default_rng(7)
    for name, h, w, seed in (("synthetic_circuit_a", 200, 260, 5), ("synthetic_circuit_b", 180, 300, 9)):
        classes = ["voltage.dc", "resistor", "transistor.bjt", "capacitor.unpolarized", "text", "diode", "gnd", "crossover", "voltage.ac", "inductor"]
        bb = []
        for k, cls in enumerate(classes):
            x, y = float(rng.integers(0, w - 40)) + 0.5 * (k % 2), float(rng.integers(0, h - 40))
            bb.append(_b(cls, x, y, x + float(rng.integers(12, 40)), y + float(rng.integers(12, 40)) + 0.25))
        out.append((name, {"gen": "circuit", "h": h, "w": w, "seed": seed}, bb))
    return out


def main():
    MG.import_reference()
    analyzer = MG.import_analyzer()
    mod = sys.modules[analyzer.__module__]
    circles = []
    mod.cv2 = stand_in_cv2(circles)
    carrier = types.SimpleNamespace(debug=True, show_image=lambda *a, **k: None, non_components={"text", "junction", "crossover", "vss", "explanatory", "circuit"},
                                    source_components={"voltage.ac", "voltage.dc", "voltage.dependent", "current.dc", "current.dependent"})
    for name in ("resize_image_keep_aspect", "resize_bboxes", "enhance_lines", "get_contours", "is_point_near_bbox"):
        setattr(carrier, name, types.MethodType(getattr(analyzer, name), carrier))

    def run(mask_spec, image_shape, bboxes):
        del circles[:]
        mask = R.golden_mask(mask_spec)
        image = np.zeros(image_shape, np.uint8) if image_shape is not None else None
        with contextlib.redirect_stdout(io.StringIO()):               # the debug prints
            got = analyzer.get_node_connections(carrier, image, mask, [dict(b) for b in bboxes])
        return R.summarize(tuple(got) + ([tuple(c) for c in circles],))
    fixture = []
    for name, spec, bboxes in cases():
        fixture.append({"name": name, "mask": spec, "image_shape": [spec["h"], spec["w"], 3], "bboxes": bboxes, "expect": run(spec, [spec["h"], spec["w"], 3], bboxes)})
    some = cases()[0][2]
    fixture.append({"name": "mask_none_with_image", "mask": None, "image_shape": [50, 70, 3], "bboxes": some, "expect": run(None, [50, 70, 3], some)})
    fixture.append({"name": "mask_none_without_image", "mask": None, "image_shape": None, "bboxes": some, "expect": run(None, None, some)})
    by = {c["name"]: c["expect"] for c in fixture}                    # the cases are what their names say
    assert sum("voltage.dc" in n["classes"] for n in by["source_on_two_nodes"]["nodes"]) == 2
    assert len(by["no_source_second_tier"]["nodes"]) == 2
    assert sorted(len(n["uids"]) for n in by["two_valid_nodes_one_single"]["nodes"]) == [1, 2]
    assert sorted(len(n["uids"]) for n in by["three_valid_nodes_single_dropped"]["nodes"]) == [2, 3]
    assert [n["uids"] for n in by["box_without_uid"]["nodes"]][0].count(None) == 1
    assert all(n["uids"].count("dup") <= 1 for n in by["two_boxes_share_a_uid"]["nodes"]) and any("dup" in n["uids"] for n in by["two_boxes_share_a_uid"]["nodes"])
    assert by["no_valid_node"]["nodes"] == [] and by["no_valid_node"]["shapes"][3] == [600, 400, 3]
    assert by["mask_none_with_image"]["shapes"] == [[50, 70, 3]] * 5 and by["mask_none_without_image"]["shapes"] == [[100, 100, 3]] * 5
    assert all(len(by[n]["nodes"]) >= 1 for n in ("synthetic_circuit_a", "synthetic_circuit_b"))
    path = os.path.join(HERE, "node_connections.json")
    with open(path, "w") as f:
        json.dump({"what": "reference control flow of get_node_connections over the project's OpenCV restatement (see make_node_golden.py)",
                   "cases": fixture}, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes,", len(fixture), "cases")


if __name__ == "__main__":
    main()
