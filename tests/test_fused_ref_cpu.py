"""The power of the fused matrix's comparison, proven without a GPU (tests/fused_ref.py, op_matrix.FUSED_ROWS): the tolerance is what the fp32
chain needs and no more, and a chain that makes one of the classic mistakes of a fused kernel violates it on the row meant to catch it."""
import pytest
import torch

from fused_ref import ATOL, C3K2_MUTANTS, CHAIN32_DEV, DWPW_MUTANTS, FACTOR, STEM2_MUTANTS, reference, row_case, tol_ratio
from helpers import TOL
from circuitvision_amd._lib import F16
from op_matrix import FUSED_MUTANT_ROWS, FUSED_ROWS

STATIC_ROWS = [r for r in FUSED_ROWS if r["B"] != "persist"]
KERNELS = ("c3k2", "stem2", "dwpw")


@pytest.fixture(scope="module")
def chain32():
    """row id -> the reference at float32, computed once."""
    out = {}
    for r in STATIC_ROWS:
        row, o, _ = row_case(r["id"])
        out[r["id"]] = reference(row, o, torch.float32)
    return out


def test_the_tolerance_is_the_measured_chain32_deviation_times_the_factor(chain32):
    """ATOL[kernel] = FACTOR x the largest |chain32 - ref64| over the kernel's non-persistent rows: the constants in fused_ref.py are this
    measurement, and every row's chain32 passes the comparison the GPU rows face."""
    for k in KERNELS:
        dev = 0.0
        for r in STATIC_ROWS:
            if r["kernel"] != k:
                continue
            ref = row_case(r["id"])[2]
            ratio, mx = tol_ratio(chain32[r["id"]], ref, k)
            assert ratio <= 1.0, (r["id"], ratio)
            assert float(ref.std()) > 0.1 and float(ref.abs().max()) < 16, f"{r['id']}: activations are meant to be O(1)"
            dev = max(dev, mx)
        print(f"{k}: largest |chain32 - ref64| {dev:.4e}  atol {ATOL[k]:.4e}")
        assert dev == CHAIN32_DEV[k], f"{k}: measured {dev!r}, fused_ref.CHAIN32_DEV says {CHAIN32_DEV[k]!r}: the rows changed, update the constant"
        assert ATOL[k] == FACTOR * dev and FACTOR == 4.0
        assert ATOL[k] < TOL[F16]["atol"] / 2, "the fused matrix is meant to bite well below the whole-model fp16 tolerance"


@pytest.mark.parametrize("mutant,rid", [(m, rid) for m, rids in FUSED_MUTANT_ROWS.items() for rid in rids])
def test_each_mutant_violates_the_tolerance_on_its_row(mutant, rid):
    row, o, ref = row_case(rid)
    ratio, mx = tol_ratio(reference(row, o, torch.float64, mutant), ref, row["kernel"])
    print(f"{mutant} on {rid}: max|err| {mx:.3e}  err/tol {ratio:.2f}")
    assert ratio > 1.0, f"{mutant} passes on {rid}: change the row (size, seed, scale), never the tolerance"


def test_every_mutant_has_rows():
    assert set(FUSED_MUTANT_ROWS) == set(C3K2_MUTANTS) | set(STEM2_MUTANTS) | set(DWPW_MUTANTS)
    by_id = {r["id"]: r for r in FUSED_ROWS}
    want = {"c3k2": C3K2_MUTANTS, "stem2": STEM2_MUTANTS, "dwpw": DWPW_MUTANTS}
    for m, rids in FUSED_MUTANT_ROWS.items():
        assert all(m in want[by_id[rid]["kernel"]] for rid in rids), m
    # the border mutants face the rows where both halos are partly outside the image, in every instance
    assert len(FUSED_MUTANT_ROWS["t_from_padded_b"]) == 10 and len(FUSED_MUTANT_ROWS["ab_bias_outside"]) == 4
    assert len(FUSED_MUTANT_ROWS["no_shortcut"]) == 5 and len(FUSED_MUTANT_ROWS["always_shortcut"]) == 5


def test_the_reference_is_deterministic_and_leaves_its_operands_alone():
    row, o, ref = row_case("c3k2_16_8_64_32_9x17")
    before = {k: v.clone() for k, v in o.items() if v is not None}
    again = reference(row, o)
    assert torch.equal(again, ref) and ref.dtype == torch.float64
    assert all(torch.equal(o[k], v) for k, v in before.items())
    assert torch.equal(ref, ref.to(torch.float16).double()), "the reference's output is an fp16 value"
