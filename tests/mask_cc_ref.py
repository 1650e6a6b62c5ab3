"""Numpy / scipy reference of the hole and sprinkle removal of SAM2Transforms.postprocess_masks (the reference's src/sam2_infer.py:88-128, with
upstream's get_connected_components).  TEST INFRASTRUCTURE ONLY.

For f32 planes x [N, h, w] and a threshold t (an f32 value): foreground is x > t, background x <= t; components are 8-connected in both
phases and never cross a plane; the label of a pixel is 1 + (y * w + x) of the raster-first pixel of its component, its area the pixel
count of its component.  The fill makes both tests on the ORIGINAL x: t + 10 where a background pixel's area <= max_hole_area (> 0),
t - 10 where a foreground pixel's area <= max_sprinkle_area (> 0), x elsewhere; the two constants are f32 sums.
[UP] the 8-connectivity of upstream's extension is its documented behaviour; the extension is not available, so it is not pinned here.
"""
import numpy as np
from scipy import ndimage as ndi

EIGHT = np.ones((3, 3), dtype=bool)
FOUR = ndi.generate_binary_structure(2, 1)


def label_plane(phase, structure=EIGHT):
    """bool [h, w] -> (labels, areas) int32 [h, w], 0 outside `phase`: label = 1 + the minimum flat index of the component."""
    lab, n = ndi.label(phase, structure=structure)
    labels, areas = np.zeros(phase.shape, np.int32), np.zeros(phase.shape, np.int32)
    if n:
        flat = lab.ravel()
        idx = np.arange(flat.size, dtype=np.int64)
        first = ndi.minimum(idx, labels=flat, index=np.arange(1, n + 1)).astype(np.int64)
        count = np.bincount(flat, minlength=n + 1)
        on = flat > 0
        labels.ravel()[on] = (first[flat[on] - 1] + 1).astype(np.int32)
        areas.ravel()[on] = count[flat[on]].astype(np.int32)
    return labels, areas


def components(x, thresh, structure=EIGHT):
    """x [N, h, w] -> (labels, areas, foreground), labels / areas int32 [N, h, w] over BOTH phases."""
    x = np.asarray(x, dtype=np.float32)
    fg = x > np.float32(thresh)
    labels, areas = np.zeros(x.shape, np.int32), np.zeros(x.shape, np.int32)
    for n in range(x.shape[0]):
        for phase in (fg[n], ~fg[n]):
            l, a = label_plane(phase, structure)
            labels[n] += l
            areas[n] += a
    return labels, areas, fg


def connected_components(mask):
    """upstream's get_connected_components contract on a bool / u8 [N, 1, H, W] array: (labels, counts), 0 on the background."""
    m = np.asarray(mask) != 0
    labels, areas = np.zeros(m.shape, np.int32), np.zeros(m.shape, np.int32)
    for n in range(m.shape[0]):
        labels[n, 0], areas[n, 0] = label_plane(m[n, 0])
    return labels, areas


def fill_small(x, thresh, max_hole_area, max_sprinkle_area, structure=EIGHT):
    """x [..., h, w] -> the filled copy (f32)."""
    x = np.asarray(x, dtype=np.float32)
    planes = x.reshape((-1,) + x.shape[-2:])
    t = np.float32(thresh)
    _, areas, fg = components(planes, t, structure)
    y = planes.copy()
    if max_hole_area > 0:
        y[~fg & (areas.astype(np.float32) <= np.float32(max_hole_area))] = t + np.float32(10)
    if max_sprinkle_area > 0:
        y[fg & (areas.astype(np.float32) <= np.float32(max_sprinkle_area))] = t - np.float32(10)
    return y.reshape(x.shape)
