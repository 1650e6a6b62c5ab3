"""CPU checks of the reference side of the e4m3 AV-product rows (tests/attn_fp8_ref.py): the bound is sharp enough to tell every wrong
variant of the arithmetic from the right one, the `exact` operands are what they claim to be, and the float64 emulation agrees with the float32
statement tests/test_ops_gpu.py has always checked the kernels against."""
import pytest
import torch

from attn_fp8_ref import FP8_MUTANTS, KINDS, LN2, V_CLAMPED, _fp8_av_emulation, c_log2, case, fp8_av_emulation, operands, score_gaps
from op_matrix import ATTN_FP8_ROWS, FP8_MUTANT_CASES

ROWS = {r["id"]: r for r in ATTN_FP8_ROWS}


def _outside(rid, kind, dt, mutant):
    """Worst |mutant - emulation| / bound over the elements (inf where the mutant is not finite)."""
    row, q, k, v, scale, c, emu, bound = case(rid, dt, kind)
    mut, _ = fp8_av_emulation(q, k, v, c, out=dt, exact_scores=(kind == "exact"), mutant=mutant)
    ratio = (mut - emu).abs() / bound
    return float(torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf"))).max())


@pytest.mark.parametrize("mutant", FP8_MUTANTS)
def test_every_mutant_is_outside_the_derived_bound_of_some_row(mutant):
    assert FP8_MUTANT_CASES.get(mutant), f"mutant {mutant}: no (row, kind, dtype) case is listed to see it"
    seen = {}
    for rid, kind, dt in FP8_MUTANT_CASES[mutant]:
        assert rid in ROWS and kind in KINDS and dt in ROWS[rid]["dtypes"], (mutant, rid, kind, dt)
        seen[(rid, kind, dt)] = _outside(rid, kind, dt, mutant)
    print(f"FP8-MUTANT {mutant}: " + ", ".join(f"{k[0]} {k[1]} {k[2]}: {v:.2f}" for k, v in seen.items()))
    assert all(v > 1.0 for v in seen.values()), f"mutant {mutant} stays inside the bound: {seen}"


def test_the_mutant_table_names_every_mutant_and_nothing_else():
    assert set(FP8_MUTANT_CASES) == set(FP8_MUTANTS), set(FP8_MUTANT_CASES) ^ set(FP8_MUTANTS)


def test_the_true_emulation_is_inside_its_own_bound_by_construction():
    """mutant=None reproduces the emulation bit for bit (the mutant switches change nothing when off)."""
    row, q, k, v, scale, c, emu, bound = case("g256_nq225_fp8", "f16", "random")
    again, b2 = fp8_av_emulation(q, k, v, c, out="f16")
    assert torch.equal(again, emu) and torch.equal(b2, bound) and bool((bound > 0).all())


@pytest.mark.parametrize("row", ATTN_FP8_ROWS, ids=[r["id"] for r in ATTN_FP8_ROWS])
def test_exact_operands_are_what_the_kind_claims(row):
    for dt in row["dtypes"]:
        q, k, v, scale, exact = operands(row, dt, "exact")
        assert exact and c_log2(scale, row["q_log2"]) == 1.0, (scale, c_log2(scale, row["q_log2"]))      # ln 2 * log2 e rounds to 1 in f32
        assert row["q_log2"] or scale == LN2
        assert float((q.abs().double() @ k.abs().double().transpose(-1, -2)).max()) < 2 ** 24              # every partial sum is exact in f32
        gaps = score_gaps(q, k)                                                                             # asserts integral scores
        assert int(gaps.min()) == 0 and int(gaps.max()) > 18, (int(gaps.min()), int(gaps.max()))           # the whole e4m3 range and beyond
        assert bool((gaps == 18).any()) and bool((gaps == 17).any()), "no key on the tie / in the lowest binade"
        v8 = v.to(torch.float8_e4m3fn).float()
        assert torch.equal(v8, v), "V is not e4m3-representable"
        assert {448.0, -448.0, 2.0 ** -9, -2.0 ** -9, 0.0} <= set(v.unique().tolist())
        # no key other than the tie sits at a boundary: the flip term of the bound is exactly the gap-18 keys' term
        qd, kd = q.double(), k.double()
        s = qd @ kd.transpose(-1, -2)
        emu, bound = fp8_av_emulation(q, k, v, 1.0, out=dt, exact_scores=True)
        x = torch.exp2(8.0 - gaps.double())
        on_grid = x.float().to(torch.float8_e4m3fn).double() == x
        assert bool((on_grid | (gaps >= 18)).all()), "a p 2^8 above the tie is not exact in e4m3"
        assert bool(torch.isfinite(emu).all()) and s.shape[-1] == row["Nk"]


@pytest.mark.parametrize("row", ATTN_FP8_ROWS, ids=[r["id"] for r in ATTN_FP8_ROWS])
def test_random_operands_exercise_the_clamp(row):
    for dt in row["dtypes"]:
        q, k, v, scale, exact = operands(row, dt, "random")
        assert not exact and int((v.abs() > 448).sum()) == V_CLAMPED and bool(torch.isfinite(v).all())
        assert (scale == 123.0) == bool(row["q_log2"])


def test_exact_kind_flip_term_is_the_tie_alone():
    """On exact operands term (1) of the bound is carried by the gap-18 keys only, and some element has such a key."""
    row, q, k, v, scale, c, emu, bound = case("dma72_fp8_256x512", "f16", "exact")
    gaps = score_gaps(q, k).reshape(q.shape[:-1] + (k.shape[-2],))
    tie_w = ((gaps == 18).double() * 2.0 ** -9 * 2.0 ** -8) @ v.double().abs()                  # un-normalised, un-rescaled: at least the term (l >= 1, alpha <= 1)
    _, flip = fp8_av_emulation(q, k, v, c, out="f16", exact_scores=True, parts=True)
    assert bool((flip <= tie_w).all()) and bool(((flip > 0) == (tie_w > 0)).all()) and float(flip.max()) > 0


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("N", [512, 1024])
def test_float64_emulation_agrees_with_the_float32_statement(dt, N):
    """The operands of test_attention_global_fp8_av_product (one (batch, head) item of them), within _check_fp8_av's tolerance vs the emulation."""
    td = torch.float16 if dt == "f16" else torch.bfloat16
    g = torch.Generator().manual_seed(19)
    q, k = (torch.randn(1, 1, N, 72, generator=g).to(td).float() for _ in range(2))
    v = (torch.randn(1, 1, N, 72, generator=g) * 1.7).to(td).float()
    scale = 72 ** -0.5
    old = _fp8_av_emulation(q, k, v, scale)
    new, bound = fp8_av_emulation(q, k, v, c_log2(scale), out=dt)
    rt = 2.0 ** -10 if dt == "f16" else 2.0 ** -7
    d = (new - old.double()).abs()
    print(f"fp8 emulation f64 vs f32, N = {N} {dt}: max {float(d.max()):.2e}; largest bound {float(bound.max()):.2e}, median {float(bound.median()):.2e}")
    assert bool((d <= 1e-2 + rt * old.abs()).all()), float(d.max())
    # ... and but for keys that the f32 statement rounds the other way, to f32 accuracy: most elements agree far below the output's rounding
    assert float((d <= 2.0 ** -16 * (1 + new.abs())).double().mean()) > 0.5
