"""The power of the resampling matrix's comparison, proven without a GPU (tests/resample_ref.py, op_matrix.RESAMPLE_ROWS): the absolute terms are
what the fp32 statements need, the exact comparisons never have to excuse an element, the fp64 statement of the antialiased resize is torch's, and a
reference that makes one of the classic mistakes of these kernels violates the bounds on the rows meant to catch it -- and only there."""
import pytest
import torch

from helper_ref import FACTOR, RTOL, SENTINEL, bilinear_ref, rT
from op_matrix import (AA_CAP_SCALE, AA_MAXTAPS, MASK_FORMS, MASK_THRESHOLDS, RECT_MAX, RESAMPLE_GRID_CAP, RESAMPLE_MUTANT_ROWS, RESAMPLE_ROWS, TRANSFORM_FORMS)
from resample_ref import (ATOL, CHAIN32_DEV, RESAMPLE_MUTANTS, aa_axis, aa_interpolate_ref, aa_transform_ref, bil_explicit, clear_of, clip_plane, clip_window,
                          extent_planes, mask_expected, mask_operands, mask_planes, mask_planes_mutant, mask_sizes, measure_chain32, tf_images, tf_items,
                          tf_mutant, tf_reference, tf_runs, tol_ratio)

BY_ID = {r["id"]: r for r in RESAMPLE_ROWS}
TF_ROWS = [r for r in RESAMPLE_ROWS if r["op"] == "transform"]
RUNNING = [r for r in TF_ROWS if tf_runs(r)]
MASK_ROWS = [r for r in RESAMPLE_ROWS if r["op"] in ("mask", "mask_sizes", "mask_rects_dev")]


def test_the_absolute_terms_are_the_measured_chain32_deviations_times_the_factor():
    dev = measure_chain32()
    assert set(dev) == set(CHAIN32_DEV) == {"aa_transform", "bilinear_edge"}
    for fam, d in sorted(dev.items()):
        print(f"{fam}: largest |chain32 - ref64| {d:.4e}  constant {CHAIN32_DEV[fam]:.4e}  atol {ATOL[fam]:.4e}")
        assert d <= CHAIN32_DEV[fam], f"{fam}: measured {d!r} is past resample_ref.CHAIN32_DEV: the rows changed, update the constant"
        assert CHAIN32_DEV[fam] <= 4 * d, f"{fam}: resample_ref.CHAIN32_DEV is more than 4 x the measured {d!r}: tighten it"
    assert FACTOR == 4.0 and all(ATOL[f] == FACTOR * CHAIN32_DEV[f] for f in CHAIN32_DEV)


def test_every_chain32_passes_the_comparison_the_gpu_rows_face():
    """f32 outputs with helper_ref's margin; a 16-bit output of the fp32 chain may round the other way next to a tie, which is one step: <= 1."""
    for row in RUNNING:
        for swap in row["swaps"]:
            ref, c32 = tf_reference(row["id"], swap), tf_reference(row["id"], swap, True)
            assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) < 3, row["id"]
            for dt in row["dtypes"]:
                ratio, _ = tol_ratio(rT(c32, dt), rT(ref, dt), "aa_transform", dt)
                assert ratio <= (1.0 / FACTOR + 0.26 if dt == "f32" else 1.0), (row["id"], swap, dt, ratio)
    for row in MASK_ROWS:
        for a, b in zip(mask_planes(row["id"], True), mask_planes(row["id"])):
            if b is not None:
                ratio, _ = tol_ratio(a, b, "bilinear_edge", "f32")
                assert ratio <= 1.0 / FACTOR + 0.26, (row["id"], ratio)
                assert bool(torch.isfinite(b).all()) and float(b.abs().max()) < 128, row["id"]


# ---- the fp64 statement is torch's --------------------------------------------------------------------------------------------------------------------
def test_the_fp64_statement_agrees_with_torch_antialiased_interpolate():
    seen = 0
    for row in RUNNING:
        if row["R"] > 64 and row["images"][0] != (8, 8):
            continue
        imgs = tf_images(row["id"])
        for b, (k, win) in list(enumerate(tf_items(row)))[:7]:
            for swap in row["swaps"]:
                d = float((tf_reference(row["id"], swap)[b] - aa_interpolate_ref(imgs[k], row["R"], win, bool(swap))).abs().max())
                assert d <= 1e-12, (row["id"], b, swap, d)
                seen += 1
    assert seen >= 40
    g = torch.Generator().manual_seed(5)
    for H, W, R in ((176, 176, 16), (64, 48, 1024), (3, 5, 48), (177, 31, 17)):      # 1 / 16 up to 11-fold down, and a non-dyadic scale
        img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).numpy()
        assert float((aa_transform_ref(img, R, stored=None) - aa_interpolate_ref(img, R)).abs().max()) <= 1e-12, (H, W, R)
    assert aa_transform_ref(img, R, stored="bf16").dtype == torch.float64 and torch.equal(aa_transform_ref(img, R, stored="bf16"), rT(aa_transform_ref(img, R, stored=None), "bf16"))


def test_the_explicit_bilinear_statement_agrees_with_torch_interpolate():
    for row in MASK_ROWS:
        low = mask_operands(row["id"])
        for n, s in enumerate(mask_sizes(row)):
            if s is not None:
                d = float((bil_explicit(low[n:n + 1], s[0], s[1]) - bilinear_ref(low[n:n + 1], s[0], s[1])).abs().max())
                assert d <= 1e-12, (row["id"], n, d)


# ---- mutants -----------------------------------------------------------------------------------------------------------------------------------------
def _tf_caught(row, mutant):
    """Largest err / bound of the mutant over the row's swaps and types, as the GPU test compares: per element, every item."""
    worst = 0.0
    for swap in row["swaps"]:
        ref, mref = tf_reference(row["id"], swap), tf_mutant(row["id"], swap, mutant)
        for dt in row["dtypes"]:
            worst = max(worst, tol_ratio(rT(mref, dt), rT(ref, dt), "aa_transform", dt)[0])
    return worst


def _mask_caught(row, mutant):
    """Does any comparison of the GPU test (f32 map under the bound, u8 mask and extent bit for bit, at every threshold) tell the mutant apart?"""
    if row["op"] == "extent":
        planes = extent_planes(row).double()
        return not torch.equal(mask_expected(planes, 0.5, mutant)[1], mask_expected(planes, 0.5)[1])
    for ref, mref in zip(mask_planes(row["id"]), mask_planes_mutant(row["id"], mutant)):
        if ref is None:
            continue
        if "bilinear_f32" in row["forms"] and tol_ratio(mref, ref, "bilinear_edge", "f32")[0] > 1.0:
            return True
        for t in row["thresholds"]:
            (m, e), (mm, me) = mask_expected(ref, t), mask_expected(mref, t, mutant)
            if not torch.equal(m, mm) or not torch.equal(e, me):
                return True
    return False


MUTANT_CASES = [(m, rid) for m, rids in RESAMPLE_MUTANT_ROWS.items() for rid in rids]


@pytest.mark.parametrize("mutant,rid", MUTANT_CASES, ids=["%s-%s" % c for c in MUTANT_CASES])
def test_each_resampling_mutant_violates_the_bounds_on_its_rows(mutant, rid):
    row = BY_ID[rid]
    if row["op"] == "transform":
        ratio = _tf_caught(row, mutant)
        print(f"{mutant} on {rid}: err/bound {ratio:.1f}")
        assert ratio > 1.0, f"{mutant} passes on {rid}: change the row, never the bound"
    else:
        assert _mask_caught(row, mutant), f"{mutant} passes on {rid}: change the row, never the comparison"


def test_only_the_rows_named_for_a_transform_mutant_see_it():
    """aa_taps_capped_16 passes every row at scale <= 7.5, aa_no_antialias every row that only up-scales, and so on: the rows are named for a reason."""
    for mutant in ("aa_taps_capped_16", "aa_no_antialias", "aa_second_window_table_restarts", "clip_moves_window"):
        for row in RUNNING:
            if row["id"] in RESAMPLE_MUTANT_ROWS[mutant] or (mutant == "aa_second_window_table_restarts" and len(row["items"]) <= RECT_MAX):
                continue
            assert _tf_caught(row, mutant) <= 1.0, (mutant, row["id"])
    for row in RUNNING:
        deep = any(max(w, h) / row["R"] > 7.5 for _, _, _, w, h in row["items"])
        assert deep == ("deep" in row["tags"]) == (row["id"] in RESAMPLE_MUTANT_ROWS["aa_taps_capped_16"]), row["id"]


def test_every_mutant_has_rows():
    assert set(RESAMPLE_MUTANT_ROWS) == set(RESAMPLE_MUTANTS)
    assert all(rids and set(rids) <= set(BY_ID) and len(rids) == len(set(rids)) for rids in RESAMPLE_MUTANT_ROWS.values())
    for m, rids in RESAMPLE_MUTANT_ROWS.items():
        ops = {BY_ID[i]["op"] for i in rids}
        assert ops <= ({"transform"} if m.startswith(("aa_", "clip_")) else {"mask", "mask_sizes", "mask_rects_dev", "extent"}), m
        if ops == {"transform"}:
            assert all(tf_runs(BY_ID[i]) for i in rids), m
    forms = lambda m: {f for i in RESAMPLE_MUTANT_ROWS[m] for f in (tf_runs(BY_ID[i]) if BY_ID[i]["op"] == "transform" else BY_ID[i]["forms"])}
    for m in ("aa_taps_capped_16", "aa_no_antialias", "aa_center_no_half", "aa_swap_moves_mean_std"):      # every form faces the mutants of the shared arithmetic
        assert forms(m) == set(TRANSFORM_FORMS), (m, forms(m))
    assert forms("aa_window_reads_image") == {"rects", "rects_dev", "srcs"} == forms("aa_second_window_table_restarts") | {"rects_dev"}
    assert forms("clip_moves_window") == {"rects_dev"}
    for m in ("bil_align_corners", "bil_no_low_clamp"):
        assert forms(m) == set(MASK_FORMS) - {"mask_extent"}, (m, forms(m))
    assert forms("bil_extent_exclusive_max") == set(MASK_FORMS)


# ---- exact comparisons never have to excuse an element -------------------------------------------------------------------------------------------------
def test_no_mask_element_sits_within_the_bound_of_its_threshold():
    planes = elements = 0
    for row in MASK_ROWS:
        assert set(row["thresholds"]) <= set(MASK_THRESHOLDS)
        for n, ref in enumerate(mask_planes(row["id"])):
            if ref is None:
                continue
            for t in row["thresholds"]:
                assert clear_of(ref, t), f"{row['id']} plane {n}: a value lies within the bilinear_edge bound of {t}: change the seed, never the comparison"
            planes, elements = planes + 1, elements + ref.numel()
    assert planes >= 150 and elements > 513 * 512                             # excused: 0 of `elements`
    flat = mask_planes("mask_empty_and_full")
    assert all(float(flat[0].max()) < t < float(flat[1].min()) for t in MASK_THRESHOLDS)
    for rid in ("mask_identity_9x7", "mask_up_2x2_to_7x5", "mask_out_1x33", "mask_out_33x1", "mask_rects_dev_513x512"):    # a blob and a background
        on = mask_planes(rid)[0] > 0.0
        assert 0.05 < float(on.float().mean()) < 0.6, rid
    a, b = (mask_planes("mask_up_2x2_to_7x5")[0] > t for t in (0.3, -1.5))
    assert not torch.equal(a, b), "the thresholds select different masks somewhere"


# ---- the rows sit where they claim to -------------------------------------------------------------------------------------------------------------------
def test_resample_rows_are_well_formed():
    ids = [r["id"] for r in RESAMPLE_ROWS]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    assert AA_CAP_SCALE == 11 and 2 * AA_CAP_SCALE + 2 == AA_MAXTAPS
    for r in TF_ROWS:
        rid, R = r["id"], r["R"]
        assert set(r["forms"]) <= set(TRANSFORM_FORMS) and r["forms"] and set(r["dtypes"]) <= {"f16", "bf16", "f32"} and set(r["swaps"]) <= {0, 1}, rid
        assert set(r["refuse"]) <= set(r["forms"]) and (not r["refuse"] or "refused" in r["tags"]), rid
        assert all(0 <= k < len(r["images"]) for k, *_ in r["items"]), rid
        whole = all((x0, y0, w, h) == (0, 0) + r["images"][k][::-1] for k, x0, y0, w, h in r["items"])
        same = len(set(r["images"])) == 1
        if {"single", "batch"} & set(r["forms"]):
            assert whole and same and [k for k, *_ in r["items"]] == list(range(len(r["images"]))), rid
        if "single" in r["forms"]:
            assert len(r["images"]) == 1, rid
        if {"rects", "rects_dev"} & set(r["forms"]):
            assert same and [k for k, *_ in r["items"]] == ([0] * len(r["items"]) if r["stride0"] else list(range(len(r["items"])))), rid
        scales = [(w / R, h / R) for _, _, w, h in (win for _, win in tf_items(r))]
        worst = max(max(s) for s in scales)
        for f in tf_runs(r):                                                   # what launches is legal: every axis of every (clipped) window at most at the cap
            assert worst <= AA_CAP_SCALE, rid
            if f == "rects_dev":
                assert max(r["images"][0]) / R <= AA_CAP_SCALE, rid
            if f != "rects_dev":
                assert all(clip_window(it[1:], *r["images"][it[0]]) == it[1:] for it in r["items"]), rid
        if "cap" in r["tags"]:                                                 # exactly at 2 * scale + 2 == AA_MAXTAPS, and the taps really reach 22
            assert 2 * worst + 2 == AA_MAXTAPS and int(aa_axis(176, R)[1].max()) >= 22, rid
        if "second_pass" in r["tags"]:
            assert R * R > RESAMPLE_GRID_CAP["transform"] and (R - 1) * (R - 1) <= RESAMPLE_GRID_CAP["transform"], rid
        if "second_table" in r["tags"] or "nothing_written" in r["tags"]:
            assert len(r["items"]) == RECT_MAX + 1 and r["items"][RECT_MAX][1:] != r["items"][0][1:], rid
    # the refusals sit one pixel past the cap, on one axis each, and the documented whole-image guard of rects_dev is pinned
    assert BY_ID["tf_refuse_177x16"]["images"] == [(177, 16)] and BY_ID["tf_refuse_16x177"]["images"] == [(16, 177)]
    assert 2 * (177 / 16) + 2 > AA_MAXTAPS >= 2 * (176 / 16) + 2
    assert BY_ID["tf_refuse_window_177_high"]["items"][0][4] == 177
    small = BY_ID["tf_small_window_in_177_high"]
    assert small["images"] == [(177, 24)] and set(small["refuse"]) == {"rects_dev"} and set(tf_runs(small)) == {"rects", "srcs"}
    assert set(BY_ID["tf_cap_window_176_in_200x300"]["forms"]) == {"rects", "srcs"}      # rects_dev would refuse the 300-wide image
    bad = BY_ID["tf_refuse_window_64_of_65"]
    assert all(clip_window(it[1:], 24, 40) == it[1:] for it in bad["items"][:64]) and clip_window(bad["items"][64][1:], 24, 40) != bad["items"][64][1:]
    clip = BY_ID["tf_clip_rects_dev"]
    kinds = [(x0 < 0, y0 < 0, x0 >= 56, w <= 0, x0 >= 0 and w > 0 and x0 < 56 and x0 + w > 56, y0 >= 0 and h > 0 and y0 + h > 40) for _, x0, y0, w, h in clip["items"]]
    assert [any(k[i] for k in kinds) for i in range(6)] == [True] * 6
    assert sum(len(r["images"]) == 3 and "batch" in r["forms"] for r in TF_ROWS) >= 1
    srcs = BY_ID["tf_srcs_three_sizes"]
    assert len(set(srcs["images"])) == 3
    # ---- the mask return
    for r in MASK_ROWS:
        assert set(r["forms"]) <= set(MASK_FORMS) and r["forms"], r["id"]
    sz = BY_ID["mask_sizes_65"]
    assert len(set(sz["sizes"])) == 65 == RECT_MAX + 1 and (1, 1) in sz["sizes"] and sz["sizes"][64] != sz["sizes"][0]
    assert BY_ID["mask_sizes_refuse_64_of_65"]["sizes"][64] == (0, 5) and BY_ID["mask_sizes_refuse_64_of_65"]["sizes"][:64] == sz["sizes"][:64]
    rd = BY_ID["mask_rects_dev_clip"]
    assert mask_sizes(rd) == [(25, 40), (1, 1000), (1, 1), (30, 33), (1, 1000)] and clip_plane((0, 0, 40, 30), 1000) == (25, 40)
    assert all(h * w <= rd["plane_stride"] for h, w in mask_sizes(rd)) and any(h * w < rd["plane_stride"] for h, w in mask_sizes(rd))
    big = BY_ID["mask_rects_dev_513x512"]
    assert mask_sizes(big) == [(513, 512)] and 513 * 512 == big["plane_stride"] > RESAMPLE_GRID_CAP["bilinear"]
    ext = BY_ID["extent_91x91"]
    assert ext["H"] * ext["W"] > RESAMPLE_GRID_CAP["mask_extent"] and [len(p) for p in ext["planes"]] == [4, 1, 0]
    assert mask_expected(extent_planes(ext).double(), 0.5)[1].tolist() == [[0, 0, 90, 90], [58, 37, 58, 37], [91, 91, -1, -1]]
    shapes = {(r["h"], r["w"], r["H"], r["W"]) for r in MASK_ROWS if r["op"] == "mask"}
    assert {(9, 7, 9, 7), (64, 64, 5, 3), (64, 64, 1, 1), (1, 1, 7, 5), (2, 2, 7, 5), (12, 10, 1, 33), (12, 10, 33, 1)} <= shapes
    assert SENTINEL == -12288.0 and RTOL["f16"] == 2.0 ** -10


def test_clip_window_and_clip_plane_state_what_the_kernels_promise():
    assert clip_window((-5, 3, 20, 10), 40, 56) == (0, 3, 20, 10)                # x0 clamped, the size kept (then clipped to what is left)
    assert clip_window((60, 5, 10, 10), 40, 56) == (55, 5, 1, 10)
    assert clip_window((10, 10, 0, -3), 40, 56) == (10, 10, 1, 1)
    assert clip_window((40, 8, 30, 12), 40, 56) == (40, 8, 16, 12) and clip_window((40, 8, 30, 12), 40, 56, "clip_moves_window") == (26, 8, 30, 12)
    assert clip_window((9, 31, 14, 25), 40, 56) == (9, 31, 14, 9)
    assert clip_plane((0, 0, 1500, 3), 1000) == (1, 1000) and clip_plane((0, 0, 0, -2), 1000) == (1, 1) and clip_plane((0, 0, 33, 30), 1000) == (30, 33)
