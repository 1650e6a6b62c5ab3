"""The power of the helper matrix's comparison, proven without a GPU (tests/helper_ref.py, op_matrix.LN_ROWS / HELPER_ROWS): the absolute terms are
what the fp32 statements need, the exact comparisons never have to excuse an element, and a reference that makes one of the classic mistakes of
these kernels violates the bounds on the rows meant to catch it."""
import pytest
import torch

from helper_ref import (ATOL, CHAIN32_DEV, CODE, FACTOR, HELPER_MUTANTS, LN_MUTANTS, SENTINEL, case, clear_of, family, ln_case, ln_grid, ln_ratio,
                        ln_reference, ln_types, measure_chain32, reference, select_ref, tol_ratio)
from op_matrix import GRID_CAP_ITEMS, HELPER_MUTANT_ROWS, HELPER_ROWS, LN_DUAL_ROWS, LN_MUTANT_ROWS, LN_ROWS, SPPF_LDS_PIXELS

BY_ID = {r["id"]: r for r in HELPER_ROWS}
LN_BY_ID = {r["id"]: r for r in LN_ROWS}


def test_the_absolute_terms_are_the_measured_chain32_deviations_times_the_factor():
    dev = measure_chain32()
    assert set(dev) == set(CHAIN32_DEV)
    for fam, d in sorted(dev.items()):
        print(f"{fam}: largest |chain32 - ref64| {d:.4e}  constant {CHAIN32_DEV[fam]:.4e}  atol {ATOL[fam]:.4e}")
        assert d <= CHAIN32_DEV[fam], f"{fam}: measured {d!r} is past helper_ref.CHAIN32_DEV: the rows changed, update the constant"
        assert CHAIN32_DEV[fam] <= 4 * d, f"{fam}: helper_ref.CHAIN32_DEV is more than 4 x the measured {d!r}: tighten it"
    assert FACTOR == 4.0 and all(ATOL[f] == FACTOR * CHAIN32_DEV[f] for f in CHAIN32_DEV if f != "dwconv3x3_f16")
    assert ATOL["dwconv3x3_f16"] == ATOL["dwconv3x3_f32"] and CHAIN32_DEV["dwconv3x3_f16"] == 0.0


def test_every_chain32_passes_the_comparison_the_gpu_rows_face():
    for row in HELPER_ROWS:
        if row["op"] not in ("refine", "dwconv3x3", "bilinear", "hyper_masks"):
            continue
        for dt in row["dtypes"]:
            _, o, ref = case(row["id"], dt)
            stored = dt if row["op"] == "dwconv3x3" else "f32"
            ratio, _ = tol_ratio(reference(row, o, dt, torch.float32), ref, family(row, dt), stored)
            assert ratio <= 1.0 / FACTOR + 0.26, (row["id"], dt, ratio)
            assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) < 128, row["id"]


# ---- mutants -----------------------------------------------------------------------------------------------------------------------------------
def _ln_caught(row, dt, mutant):
    """Does the GPU test's comparison (values under the LayerNorm bounds, untouched padding rows) tell the mutant from the reference?"""
    _, o, ref, scale = ln_case(row["id"], dt)
    dout = CODE[ln_types(row, dt)[1]]
    mref, _ = ln_reference(row, o, mutant)
    want, got = ln_grid(row, ref, SENTINEL), ln_grid(row, mref, SENTINEL, mutant)
    valid = want != SENTINEL
    if bool(((got == SENTINEL) != ~valid).any()):
        return True, float("inf")
    ratio, _ = ln_ratio(got[valid], want[valid], ln_grid(row, scale, 1.0)[valid], dout)
    return ratio > 1.0, ratio


@pytest.mark.parametrize("mutant,rid", [(m, rid) for m, rids in LN_MUTANT_ROWS.items() for rid in rids])
def test_each_layernorm_mutant_violates_the_bounds_on_its_rows(mutant, rid):
    row = LN_BY_ID[rid]
    for dt in row["dtypes"]:
        caught, ratio = _ln_caught(row, dt, mutant)
        print(f"{mutant} on {rid} {dt}: err/bound {ratio:.2f}")
        assert caught, f"{mutant} passes on {rid} {dt}: change the row, never the bound"


def test_only_rows_with_idle_slots_catch_statistics_over_every_slot():
    full = [r for r in LN_ROWS if r["waste"] == 0 and not r["pad"]]
    assert len(full) >= 20
    for row in full[::7]:
        assert not _ln_caught(row, row["dtypes"][0], "ln_stats_over_slots")[0], row["id"]


@pytest.mark.parametrize("mutant,rid", [(m, rid) for m, rids in HELPER_MUTANT_ROWS.items() for rid in rids])
def test_each_helper_mutant_violates_the_bounds_on_its_rows(mutant, rid):
    row = BY_ID[rid]
    for dt in row["dtypes"]:
        _, o, ref = case(rid, dt)
        mref = reference(row, o, dt, torch.float64, mutant)
        if row["op"] == "sppf_pool":                                     # exact comparison
            assert not torch.equal(mref, ref), f"{mutant} passes on {rid} {dt}"
            continue
        ratio, mx = tol_ratio(mref, ref, family(row, dt), dt if row["op"] == "dwconv3x3" else "f32")
        print(f"{mutant} on {rid} {dt}: max|err| {mx:.3e}  err/tol {ratio:.2f}")
        assert ratio > 1.0, f"{mutant} passes on {rid} {dt}: change the row (size, seed, scale), never the tolerance"


def test_every_mutant_has_rows():
    assert set(LN_MUTANT_ROWS) == set(LN_MUTANTS) and set(HELPER_MUTANT_ROWS) == set(HELPER_MUTANTS)
    assert all(rids and set(rids) <= set(LN_BY_ID) for rids in LN_MUTANT_ROWS.values())
    assert all(rids and set(rids) <= set(BY_ID) for rids in HELPER_MUTANT_ROWS.values())
    forms = {r["form"] for r in LN_ROWS}
    for m, rids in LN_MUTANT_ROWS.items():                               # every form faces every LayerNorm mutant, at NCH = 3 and at another instance
        for f in forms:
            assert {LN_BY_ID[i]["NCH"] for i in rids if LN_BY_ID[i]["form"] == f} >= {3, 2}, (m, f)


# ---- exact comparisons never have to excuse an element ------------------------------------------------------------------------------------------
def test_no_mask_element_sits_within_the_bound_of_the_threshold():
    row = BY_ID["mask_postprocess_520x517"]
    _, o, ref = case(row["id"], "f32")
    assert torch.equal(ref, case("bilinear_520x517", "f32")[2]), "both rows resize the same map"
    assert clear_of(ref, 0.0), "an interpolated value lies within the bilinear bound of the threshold: change the seed, never the comparison"
    on = ref > 0.0
    assert all(0.05 < float(on[n].float().mean()) < 0.6 for n in range(row["N"])), "every plane holds a blob and a background"


def test_no_mask0_value_sits_within_the_bound_of_delta_and_one_image_falls_back():
    for row in (r for r in HELPER_ROWS if r["op"] == "hyper_masks"):
        for dt in row["dtypes"]:
            _, o, ref = case(row["id"], dt)
            assert clear_of(ref[:, 0], row["delta"], "hyper_masks") and clear_of(ref[:, 0], -row["delta"], "hyper_masks"), (row["id"], dt)
            areas, sel, stab = select_ref(ref, o["iou"], row["delta"], row["thresh"])
            assert sel.tolist()[0] == 0 and sel.tolist()[2] == 0 and sel.tolist()[1] in (1, 2, 3), (row["id"], dt, sel, stab)
            assert bool(((stab - row["thresh"]).abs() > 5e-3).all()), "a stability score next to the threshold: fp32 rounding may flip the selection"
            assert bool((areas[:, 1] > 0).all())


# ---- the rows sit where they claim to ------------------------------------------------------------------------------------------------------------
def test_helper_rows_are_well_formed():
    ids = [r["id"] for r in HELPER_ROWS] + [r["id"] for r in LN_ROWS] + [r["id"] for r in LN_DUAL_ROWS]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    for r in HELPER_ROWS:
        op, rid = r["op"], r["id"]
        if op == "sppf_pool":
            vec = 4 if r["dtypes"] == ("f32",) else 8
            assert r["B"] >= 2 and r["C"] >= 2 * vec and r["C"] % vec == 0 and r["ld"] >= 4 * r["C"] and r["ld"] % vec == 0, rid
        elif op == "cast":
            assert r["rows"] * r["C"] > GRID_CAP_ITEMS[op], rid
        elif op == "maxpool2x2":
            assert r["B"] * (r["H"] // 2) * (r["W"] // 2) * (r["C"] // (4 if r["dtypes"] == ("f32",) else 8)) > GRID_CAP_ITEMS[op], rid
        elif op == "space_to_depth4":
            assert r["B"] * (r["H"] // 4) * (r["W"] // 4) * 4 > GRID_CAP_ITEMS[op], rid
        elif op in ("nchw_to_nhwc", "nhwc_to_nchw_f32"):
            assert r["B"] * r["C"] * r["H"] * r["W"] > GRID_CAP_ITEMS[op], rid
        elif op == "repeat_images":
            assert r["chunks"] > GRID_CAP_ITEMS[op] and r["rep"] == 3, rid
        elif op in ("bilinear", "mask_postprocess"):
            assert r["H"] * r["W"] > GRID_CAP_ITEMS["bilinear"], rid
        elif op == "hyper_masks":
            assert r["P"] > GRID_CAP_ITEMS[op] and r["up_ld"] > r["C"] and r["B"] == 3, rid
        elif op == "dwconv3x3":
            assert r["B"] == 3 and r["x_off"] == 8 and r["y_guard"] == 8, rid
    second = BY_ID["sppf_second_pass_f16"]
    assert second["B"] * second["H"] * second["W"] * (second["C"] // 8) > GRID_CAP_ITEMS["sppf_pool"] and second["expect"].startswith("sppf_pool_kernel<")
    for dt, px in SPPF_LDS_PIXELS.items():
        at, past = BY_ID["sppf_lds_limit_" + dt], BY_ID["sppf_past_lds_limit_" + dt]
        assert at["H"] * at["W"] == px and at["expect"].startswith("sppf_pool_lds_kernel<")
        assert past["H"] * past["W"] == px + at["W"] and past["expect"].startswith("sppf_pool_kernel<")
    assert any(r["op"] == "sppf_pool" and r["ld"] > 4 * r["C"] for r in HELPER_ROWS)
    for r in LN_ROWS:
        vi = 4 if r["form"].startswith("f32") else 8
        assert r["C"] % vi == 0 and r["x_ld"] % vi == 0 and r["y_ld"] % vi == 0 and r["x_off"] % 8 == 0 and r["y_off"] % 8 == 0, r["id"]
        if r["form"] == "f32_16w":
            assert r["C"] % 8 == 0 and r["y_ld"] % 8 == 0, r["id"]
        if r["form"] == "f32_16n":
            assert r["C"] % 8 == 4 or r["y_ld"] % 8 == 4, r["id"]
        assert r["rows"] <= 400 and (not r["pad"] or r["rows"] % (r["pad"][0] * r["pad"][1]) == 0), r["id"]
    assert {r["NCH"] for r in LN_DUAL_ROWS} == {1, 3, 9}
