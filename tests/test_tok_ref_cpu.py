"""The power of the token-path matrix's comparison, proven without a GPU (tests/tok_ref.py, op_matrix.TOK_ROWS / MLP_ROWS): the bounds are what a
correct fp32 implementation needs and no more, and a reference that makes one of the classic mistakes of a token-stationary kernel -- a stale ring
slot, a split launch's ring origin, a dropped last piece, a written guard, the Chan combination without its second term, a pool grid read with the
wrong width -- violates them on every row meant to catch it."""
import pytest
import torch

from op_matrix import (FAR500_MUTANTS, KIND_BLOCKS, KIND_ROWS, MLP_KIND_MUTANT_ROWS, MLP_KIND_ROWS, MLP_ROWS, PROJ_MUTANT_ROWS, PROJ_ROWS, TOK_MUTANT_DTYPES,
                       TOK_MUTANT_ROWS, TOK_ROWS, TOK_UNSEEN_MUTANTS)
from tok_ref import (ALL_ROWS, ATOL, CHAIN32_DEV, FACTOR, HAND_SET, MLP_KIND_MUTANTS, MLP_MUTANTS, PROJ_MUTANTS, RTOL, STATS_PAIR_TOL, TOK_MUTANTS, TDT, family,
                     gelu_form_error, judge, measure, measure_kinds, reference, row_case, stats_ref, stored)

DTS = ("f16", "bf16")
# families whose measured bound is NOT below half of today's hand-set tolerance (tests/test_ops_gpu.py), with the reason: all are set by
# the error of the GELU form the kernels evaluate, which chain32 reproduces (tok_ref.gelu_fast) -- see test_the_gelu_form_error_is_what_was_measured
OVER_HALF_OF_HAND_SET = {("gelu_ln", "f16"), ("mlp", "f16"), ("mlp", "bf16"), ("mlp_kinds", "f16"), ("mlp_kinds", "bf16"), ("projmlp", "f16"), ("projmlp", "bf16")}


@pytest.fixture(scope="module")
def measured():
    return measure(DTS)


def test_the_tolerance_is_the_measured_chain32_deviation_times_the_factor(measured):
    """ATOL[family, dtype] = FACTOR x the largest |chain32 - ref64| over the family's rows: the constants in tok_ref.py are this measurement (the
    16-bit families' exactly: whole steps of the stored type; the f32 families' rounded up, never more than 1.25 x loose)."""
    dev, _ = measured
    assert set(dev) == set(CHAIN32_DEV) == set(ATOL) and FACTOR == 4.0
    for k in sorted(dev):
        print(f"{k[0]} {k[1]}: largest |chain32 - ref64| {dev[k]:.4e}  constant {CHAIN32_DEV[k]:.4e}  atol {ATOL[k]:.4e}")
        assert dev[k] <= CHAIN32_DEV[k] <= 1.25 * dev[k], f"{k}: measured {dev[k]!r}, tok_ref.CHAIN32_DEV says {CHAIN32_DEV[k]!r}: the rows changed, update the constant"
        if k[0].startswith(("o16", "gelu")):
            assert dev[k] == CHAIN32_DEV[k], k
        assert ATOL[k] == FACTOR * CHAIN32_DEV[k]
        hand = HAND_SET[k[0].split("_")[0], k[1]]
        assert (ATOL[k] < hand / 2) == (k not in OVER_HALF_OF_HAND_SET), f"{k}: atol {ATOL[k]:.3e} against half of the hand-set {hand:.1e}"
    assert RTOL == {"f16": 2.0 ** -10, "bf16": 2.0 ** -7, "f32": 0.0}


def test_no_family_loosens_another_k_by_more_than_twice(measured):
    _, per_k = measured
    """No K of a family is held to a bound more than twice what its own rows measure (else the family would have to be split); for the 16-bit
    families, whose deviations are whole steps of the stored type, a factor 2 is one binade."""
    for (fam, K, dt), v in per_k.items():
        assert CHAIN32_DEV[fam, dt] <= 2 * v, (fam, K, dt, v)


@pytest.mark.parametrize("dt", DTS)
def test_every_rows_chain32_passes_the_comparison_the_gpu_rows_face(dt):
    for rid, row in ALL_ROWS.items():
        _, o, ref = row_case(rid, dt)
        c32 = reference(row, o, dt, torch.float32)
        ratio, _, fails = judge(row, dt, o, ref, c32["out"], c32["stats"])
        assert not fails and ratio <= 1.0 / FACTOR + 1e-9, (rid, dt, ratio, fails)
        n = row.get("N", row.get("C"))
        whole = ref["out"][:, :n] if row.get("proj") else ref["out"]       # (the proj rows' padding columns are NaN before and after)
        big = 600.0 if row.get("kinds") else 16.0                         # (the kinds rows sit up to 500 away from zero on purpose)
        assert bool(torch.isfinite(whole).all()) and float(ref["out"][:, :n].abs().max()) < (2.0 if stored(row, dt) != "f32" else big), rid


@pytest.mark.parametrize("mutant,rid,dt", [(m, rid, dt) for m, rids in TOK_MUTANT_ROWS.items() for rid in rids for dt in TOK_MUTANT_DTYPES.get(m, DTS)])
def test_each_mutant_violates_the_tolerance_on_its_row(mutant, rid, dt):
    row, o, ref = row_case(rid, dt)
    mo = reference(row, o, dt, torch.float64, mutant)
    ratio, mx, fails = judge(row, dt, o, ref, mo["out"], mo["stats"])
    print(f"{mutant} on {rid} {dt}: max|err| {mx:.3e}  err/bound {ratio:.2f}  {fails}")
    assert fails, f"{mutant} passes on {rid} ({dt}): change the row (size, seed, scale), never the tolerance"


NEW_MUTANT_CASES = [(m, rid, dt) for table in (PROJ_MUTANT_ROWS, MLP_KIND_MUTANT_ROWS) for m, rids in table.items() for rid in rids for dt in DTS]


@pytest.mark.parametrize("mutant,rid,dt", NEW_MUTANT_CASES)
def test_each_proj_and_kinds_mutant_violates_the_tolerance_on_its_row(mutant, rid, dt):
    """PROJ_MUTANT_ROWS / MLP_KIND_MUTANT_ROWS, fp16 and bf16.  The two raw-moment mutants must fall on the rows 500 away from zero: judged on
    those KIND_ROWS rows alone (output columns and statistics), they are outside the bound there."""
    row, o, ref = row_case(rid, dt)
    mo = reference(row, o, dt, torch.float64, mutant)
    ratio, mx, fails = judge(row, dt, o, ref, mo["out"], mo["stats"])
    print(f"{mutant} on {rid} {dt}: max|err| {mx:.3e}  err/bound {ratio:.2f}  {fails}")
    assert fails, f"{mutant} passes on {rid} ({dt}): change the row (size, seed, scale), never the tolerance"
    if mutant in FAR500_MUTANTS:
        assert row["kinds"] and KIND_BLOCKS[0] == "far500"
        C, far = row["C"], slice(0, KIND_ROWS)
        if mutant == "ln_var_raw_moments":
            err = (mo["out"][far, :C] - ref["out"][far, :C]).abs().max()
            assert float(err) > ATOL[family(row), dt], (rid, dt, float(err))
        else:
            exp = stats_ref(mo["out"][far], C)
            off = ((mo["stats"][far].double() - exp).abs() / (STATS_PAIR_TOL[1] + STATS_PAIR_TOL[0] * exp.abs())).max()
            assert float(off) > 1.0, (rid, dt, float(off))


def test_the_kinds_do_not_call_for_a_family_of_their_own(measured):
    """A kinds family is split off its launch's family only when its constant exceeds 2 x the plain mlp constant; neither does, so the kinds
    rows of proj_mlp stay in projmlp, and no kind of either family deviates by more than 2 x what the plain rows of the same launch do."""
    dev, _ = measured
    for dt in DTS:
        assert CHAIN32_DEV["mlp_kinds", dt] <= 2 * CHAIN32_DEV["mlp", dt] and CHAIN32_DEV["projmlp", dt] <= 2 * CHAIN32_DEV["mlp", dt], dt
    per_kind = measure_kinds(DTS)
    assert {k[0] for k in per_kind} == {r["id"] for r in MLP_KIND_ROWS + PROJ_ROWS if r.get("kinds")}
    for (rid, dt), v in sorted(per_kind.items()):
        print(f"{rid} {dt}: " + "  ".join(f"{k} {x:.3e}" for k, x in zip(KIND_BLOCKS + ("plain",), v)))
        assert max(v[:-1]) <= 2 * CHAIN32_DEV["mlp", dt], (rid, dt, v)


def test_every_proj_and_kinds_mutant_has_rows():
    assert set(PROJ_MUTANT_ROWS) == set(PROJ_MUTANTS) and set(MLP_KIND_MUTANT_ROWS) == set(MLP_KIND_MUTANTS)
    proj_ids, kind_ids = {r["id"] for r in PROJ_ROWS}, {r["id"] for r in MLP_KIND_ROWS}
    for m, rids in PROJ_MUTANT_ROWS.items():
        assert rids and set(rids) <= proj_ids, m
        assert {ALL_ROWS[rid]["expect"] for rid in rids} == {"proj_mlp_kernel<144, 1>", "proj_mlp_kernel<288, 2>"}, m      # ... on both instances
    for m, rids in MLP_KIND_MUTANT_ROWS.items():
        assert set(rids) == kind_ids, m
    for m in FAR500_MUTANTS:
        assert all(ALL_ROWS[rid]["kinds"] for rid in PROJ_MUTANT_ROWS[m] + MLP_KIND_MUTANT_ROWS[m]), m
    assert set(PROJ_MUTANT_ROWS["proj_rows_past_end"]) == {r["id"] for r in PROJ_ROWS if r["rows"] % 128}
    assert set(PROJ_MUTANT_ROWS["stats_of_x1"]) == {r["id"] for r in PROJ_ROWS if r["stats_out"]}
    assert not (set(PROJ_MUTANTS) | set(MLP_KIND_MUTANTS)) & set(TOK_UNSEEN_MUTANTS)      # every one of them is caught: no new blind spot


def test_every_mutant_has_rows():
    assert set(TOK_MUTANT_ROWS) | set(TOK_UNSEEN_MUTANTS) == set(TOK_MUTANTS) | set(MLP_MUTANTS) and not set(TOK_MUTANT_ROWS) & set(TOK_UNSEEN_MUTANTS)
    for m, rids in list(TOK_MUTANT_ROWS.items()) + list(TOK_UNSEEN_MUTANTS.items()):
        assert rids and set(rids) <= set(ALL_ROWS), m
        assert all(("C" in ALL_ROWS[rid]) == (m in MLP_MUTANTS) for rid in rids), m
        assert set(TOK_MUTANT_DTYPES.get(m, DTS)) <= set(DTS) and TOK_MUTANT_DTYPES.get(m, DTS)
    ks = lambda m: {ALL_ROWS[rid]["K"] for rid in TOK_MUTANT_ROWS[m]}
    for m in ("ring_stale_slot", "last_piece_dropped", "guard_written", "res_overwrite", "ln_no_eps", "chan_no_between_term", "chan_raw_moments", "stats_over_ld",
              "pool_dxdy_swapped", "pool_w_for_hw", "pool_mean"):
        assert ks(m) == {144, 288, 576}, m                                  # ... at every K
    assert {ALL_ROWS[rid]["stats_in"] for rid in TOK_MUTANT_ROWS["chan_no_between_term"]} == {2, 3, 6}
    assert {ALL_ROWS[rid]["ns"] for rid in TOK_MUTANT_ROWS["split_ring_origin"]} == {2, 3, 4, 5, 6, 7, 8}
    assert any(ALL_ROWS[rid]["grid"] == (2, 64, 6) for rid in TOK_MUTANT_ROWS["pool_w_for_hw"])


@pytest.mark.parametrize("dt", DTS)
def test_the_blind_spot_is_what_was_measured(dt):
    """mlp_hidden_not_rounded stays below the bound on every row (it is more accurate than the contract, by less than the GELU form's error):
    recorded here so that a tighter MLP bound, should one become possible, is noticed."""
    worst = 0.0
    for rid in TOK_UNSEEN_MUTANTS["mlp_hidden_not_rounded"]:
        row, o, ref = row_case(rid, dt)
        mo = reference(row, o, dt, torch.float64, "mlp_hidden_not_rounded")
        ratio, _, fails = judge(row, dt, o, ref, mo["out"], mo["stats"])
        assert not fails, (rid, fails)
        worst = max(worst, ratio)
    print(f"mlp_hidden_not_rounded {dt}: worst err/bound {worst:.3f}")
    assert worst < (0.12 if dt == "f16" else 0.6)


def test_the_gelu_form_error_is_what_was_measured():
    """The documented sigmoid(x P(x^2)) form against the exact GELU on every fp16 value of [-8, 8].  f32 arithmetic (gelu_fast, the bf16 build):
    2.5e-5 absolute, as common.hpp says.  Packed fp16 arithmetic (gelu_fast_pk, the fp16 build): up to 3.4e-3 relative on 0.5 <= |x| <= 2 --
    common.hpp's comment says 1e-3 around |x| ~ 1 -- because the exponent x P(x^2) is itself rounded to fp16 (a step of 2^-9 .. 2^-8 at 2 .. 8)."""
    a16, mid16, _ = gelu_form_error("f16")
    a32, mid32, _ = gelu_form_error("bf16")
    print(f"gelu_fast_pk: max|err| {a16:.3e}, relative on 0.5 <= |x| <= 2 {mid16:.3e};  gelu_fast: {a32:.3e}, {mid32:.3e}")
    assert a32 <= 2.6e-5 and mid32 <= 6e-4
    assert 3.0e-3 <= mid16 <= 3.6e-3 and a16 <= 2.5e-3


def test_the_references_are_deterministic_and_leave_their_operands_alone():
    for rid in ("k288_ln1_gelu_n136_ld144_nch", "k576_ln0_res_n576_ld576_split6_parts_out", "k144_pool_n36_ld40_grid2x64x6", "mlp_c288_v2_rows391_ld292"):
        for dt in DTS:
            row, o, ref = row_case(rid, dt)
            before = {k: v.clone() for k, v in o.items() if v is not None}
            again = reference(row, o, dt)
            assert torch.equal(again["out"], ref["out"]) and ref["out"].dtype == torch.float64
            assert (again["stats"] is None) == (ref["stats"] is None) and (ref["stats"] is None or torch.equal(again["stats"], ref["stats"]))
            assert all(torch.equal(o[k], v) or bool(torch.isnan(v).any()) for k, v in before.items())


@pytest.mark.parametrize("dt", DTS)
def test_reference_outputs_of_16_bit_forms_are_16_bit_values(dt):
    n = 0
    for r in TOK_ROWS:
        if stored(r, dt) == "f32":
            continue
        _, o, ref = row_case(r["id"], dt)
        y = ref["out"][:, :r["N"]]
        assert torch.equal(y, y.to(TDT[dt]).double()), r["id"]
        assert torch.equal(o["w"], o["w"].to(TDT[dt]).float()) and (r["ln"] != 0 or torch.equal(o["x"], o["x"].to(TDT[dt]).float())), r["id"]
        n += 1
    assert n > 80
