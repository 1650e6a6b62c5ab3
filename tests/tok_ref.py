"""Plain references of the token-stationary kernels (tok_linear.hip, tok_linear16.hip, hiera_mlp.hip and its proj form, proj_mlp.hpp), the seeded
operands of every row of op_matrix.TOK_ROWS / MLP_ROWS / MLP_KIND_ROWS / PROJ_ROWS and the bounds the token-path matrix
(tests/test_tok_matrix_gpu.py) holds the kernels to.  CPU only, plain torch: importing this module needs neither a GPU nor the library.

The references state the op in `dtype` on operands that arrive pre-rounded to the operand type ("f16" | "bf16") and round exactly where the
kernels' contracts say a 16-bit value is formed: the LayerNorm output (the MFMA's B fragments), the 16-bit output, the MLP's hidden activation.
The f32 residual path is not rounded.  The bias of the 32x32x16 format (K = 144 / 288, and the MLP's fc1) is what the packed weights carry: the
hi + lo pair of PackedTokLinear / PackedHieraMlp, recomputed here by the same two roundings; K = 576 and the MLP's fc2 read the exact f32 bias.
dtype = float64 with the exact erf GELU is the yardstick.  The same statement at float32 ("chain32") stands for an implementation that is right
but accumulates in fp32; where the row has a GELU, chain32 evaluates the documented sigmoid(x P(x^2)) form of gelu_fast / gelu_fast_pk
(common.hpp) -- in fp16 arithmetic for the fp16 build, f32 for bf16 -- so the approximation's own error is part of the calibration.
mutant= selects one deliberately wrong statement, so that tests/test_tok_ref_cpu.py can prove without a GPU that rows and bounds catch it.

pool_dxdy_swapped: exchanging (dy, dx) alone makes the lane quad visit the same four tokens, which a maximum cannot see; the mutant here is the
nearest mistake that can show -- both offsets taken from the same lane bit, so the quad covers the block's diagonal only.

`PYTHONPATH=. python tests/tok_ref.py` (from the repository root) prints the measured chain32 deviations behind CHAIN32_DEV and the GELU form's
error against the exact GELU."""
import functools
import zlib

import torch
import torch.nn.functional as F

from op_matrix import KIND_BLOCKS, KIND_ROWS, MLP_KIND_ROWS, MLP_ROWS, PROJ_ROWS, TOK_FORMAT, TOK_ROWS, tl16_splits

TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
SENT16 = -12288.0                                      # guard value of 16-bit outputs: exact in fp16 and bf16
SENT32 = 1.0e4                                         # guard value of f32 outputs (residual stream, pooled map, the MLP's padding columns)
LN_EPS = 1e-6
WSCALE = 0.125                                         # 16-bit outputs stay below 1 but for a few near it: one step of the stored type is 2^-11 (fp16) / 2^-8 (bf16) or less

TOK_MUTANTS = ("ring_stale_slot", "split_ring_origin", "last_piece_dropped", "guard_written", "res_overwrite", "ln_no_eps", "ln_var_n_minus_1",
               "chan_no_between_term", "chan_raw_moments", "stats_over_ld", "pool_dxdy_swapped", "pool_w_for_hw", "pool_mean", "bias_hi_only")
MLP_MUTANTS = ("mlp_hidden_not_rounded", "mlp_rows_past_end")
MLP_KIND_MUTANTS = ("ln_var_raw_moments", "stats_unshifted")
PROJ_MUTANTS = ("proj_bias_twice", "proj_bias_not_in_ln", "ln_of_x_not_x1", "residual_drops_proj", "fc1_k_natural_order", "proj_rows_past_end", "stats_of_x1",
                "ln_var_raw_moments", "stats_unshifted", "x1_through_16_bits")

# |y - ref64| <= ATOL[family, dtype] + RTOL[stored type] |ref64| per element.  RTOL is one step of the stored output (0 for f32 outputs).
# ATOL = FACTOR x the largest |chain32 - ref64| over the rows of the family, measured on the CPU (main() below) and re-measured by
# tests/test_tok_ref_cpu.py, which fails when a row change moves a measurement past its constant or leaves the constant more than 1.25 x too
# loose.  The factor is the project's margin for what chain32 does not reproduce: the MFMA summation order, v_rcp / v_exp, the shifted
# single-pass variance.  No kernel enters these numbers.
RTOL = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7, "f32": 0.0}
FACTOR = 4.0
# measured largest |chain32 - ref64| per (family, dtype), rounded up to two digits.  Families: the 16-bit output without / with GELU, the f32
# residual form, the pooled f32 map and the fused MLP, each split by whether a LayerNorm feeds the MFMA ("_ln": the fp32 LayerNorm may round
# a B-fragment value the other way, one operand step times a weight) or the operands arrive exact ("_raw").
#   o16_raw   f16 2^-12  bf16 2^-9     one step of an output in [0.25, 0.5) that the fp32 accumulation rounds the other way
#   o16_ln    f16 2^-11  bf16 2^-8     ... of an output in [0.5, 1)
#   gelu_raw  f16 2^-11  bf16 2^-9     the GELU form's error (gelu_form_error below) moves more outputs across a tie
#   gelu_ln   f16 2^-10  bf16 2^-8     fp16: two steps of an output in [0.5, 1) -- gelu_fast_pk's fp16 arithmetic
#   res_raw   f16 4.5e-7 bf16 3.0e-7   f32 accumulation and the f32 addition to an O(1) stream
#   res_ln    f16 9.8e-5 bf16 4.4e-4   a B-fragment value rounded the other way, times a weight
#   pool      f16 6.8e-5 bf16 4.4e-4   the same, through the maximum
#   mlp       f16 1.9e-3 bf16 3.3e-3   fp16: 1152 hidden values each carrying gelu_fast_pk's error (up to 3e-3 relative), summed by fc2
CHAIN32_DEV = {
    ("o16_raw", "f16"): 2.0 ** -12, ("o16_raw", "bf16"): 2.0 ** -9, ("o16_ln", "f16"): 2.0 ** -11, ("o16_ln", "bf16"): 2.0 ** -8,
    ("gelu_raw", "f16"): 2.0 ** -11, ("gelu_raw", "bf16"): 2.0 ** -9, ("gelu_ln", "f16"): 2.0 ** -10, ("gelu_ln", "bf16"): 2.0 ** -8,
    ("res_raw", "f16"): 4.7e-7, ("res_raw", "bf16"): 3.2e-7, ("res_ln", "f16"): 1.0e-4, ("res_ln", "bf16"): 4.6e-4,
    ("pool", "f16"): 7.1e-5, ("pool", "bf16"): 4.6e-4, ("mlp", "f16"): 2.0e-3, ("mlp", "bf16"): 3.4e-3,
    #   mlp_kinds f16 2.1e-3 bf16 4.2e-3   fp16: as mlp (the last-channel outlier rows); bf16: the rows 500 away from zero -- the f32 mean of 144 / 288 values
    #                                      near 500 is off by 1e-5 of their spread, and more B-fragment values round the other way
    #   projmlp   f16 1.9e-3 bf16 4.3e-3   fp16: as mlp (a plain row); bf16: the 1e-3-spread rows -- x + ao Wp^T formed in f32 moves x1 by 1e-7, 1e-4 of
    #                                      that spread, ahead of the same rounding
    # Neither is above 2 x the plain mlp constant: the kinds rows stay in their launch's family (main() prints the deviation per kind).
    ("mlp_kinds", "f16"): 2.2e-3, ("mlp_kinds", "bf16"): 4.2e-3, ("projmlp", "f16"): 1.9e-3, ("projmlp", "bf16"): 4.4e-3,
}
ATOL = {k: FACTOR * v for k, v in CHAIN32_DEV.items()}
# today's hand-set absolute tolerances of tests/test_ops_gpu.py for the same forms (16-bit output, f32 residual, pooled map, fused MLP)
HAND_SET = {("o16", "f16"): 4e-3, ("o16", "bf16"): 3.2e-2, ("gelu", "f16"): 4e-3, ("gelu", "bf16"): 3.2e-2, ("res", "f16"): 3e-3, ("res", "bf16"): 2.4e-2,
            ("pool", "f16"): 4e-3, ("pool", "bf16"): 3.2e-2, ("mlp", "f16"): 3e-3, ("mlp", "bf16"): 2.4e-2,
            ("projmlp", "f16"): 3e-3, ("projmlp", "bf16"): 2.4e-2}          # (projmlp: tests/test_proj_mlp_gpu.py)
STATS_PAIR_TOL = (2e-5, 2e-5)                          # (rtol, atol) of forwarded (mean, rstd) against the rows as written
STATS_PARTS_TOL = (1e-4, 1e-3)                         # ... of per-slice (mean, sum of squared deviations)


def rT(t, dt):
    """Round to the 16-bit type dt and come back: the places where a kernel forms a 16-bit value."""
    return t.to(TDT[dt]).to(t.dtype)


def family(row):
    if "C" in row:
        return "projmlp" if row.get("proj") else "mlp_kinds" if row.get("kinds") else "mlp"
    if row["pool"]:
        return "pool"
    return ("res" if row["res"] else "gelu" if row["gelu"] else "o16") + ("_ln" if row["ln"] == 1 else "_raw")


def stored(row, dt):
    return dt if "K" in row and not (row["res"] or row["pool"]) else "f32"


def _gen(rid, dt):
    return torch.Generator().manual_seed(zlib.crc32((rid + dt).encode()))


# ---- GELU ---------------------------------------------------------------------------------------------------------------------------------------
GELU_P = (1.01426788e-03, -1.06775760e-01, -2.30112128e+00)     # common.hpp gelu_fast: P(s) = (P[0] s + P[1]) s + P[2], carries -log2(e)


def gelu_fast(v, dt):
    """common.hpp's x * sigmoid(x P(x^2)) on a float32 tensor: gelu_fast_pk's packed fp16 arithmetic (every operation rounded to fp16, the two
    v_pk_fma with one rounding each) for dt = "f16", gelu_fast's f32 arithmetic for "bf16".  The caller rounds the result to the stored type."""
    v = v.float()
    if dt == "f16":
        h = lambda t: t.to(torch.float16).float()
        c2, c1, c0 = (h(torch.tensor(c)) for c in GELU_P)
        v = h(v)
        s = torch.clamp(h(v * v), max=64.0)
        pl = h(s * h(s * c2 + c1) + c0)
        d = h(h(torch.exp2(h(v * pl))) + 1.0)
        return h(v * h(1.0 / d))
    s = torch.clamp(v * v, max=64.0)
    pl = s * (s * GELU_P[0] + GELU_P[1]) + GELU_P[2]
    return v * (1.0 / (1.0 + torch.exp2(v * pl)))


def _gelu(y, dt, fast):
    return gelu_fast(y, dt).to(y.dtype) if fast else F.gelu(y)


def gelu_form_error(dt):
    """(largest |gelu_fast - GELU|, largest relative error over 0.5 <= |x| <= 2, ... over 2^-6 <= |x| <= 8) on every fp16 value of [-8, 8]."""
    x = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16).view(torch.float16).float()
    x = x[torch.isfinite(x) & (x.abs() <= 8)]
    err = (gelu_fast(x, dt).double() - F.gelu(x.double())).abs()
    rel = err / F.gelu(x.double()).abs().clamp(min=1e-300)
    mid, wide = (x.abs() >= 0.5) & (x.abs() <= 2), x.abs() >= 2.0 ** -6
    return float(err.max()), float(rel[mid].max()), float(rel[wide & (x > -3)].max())


# ---- LayerNorm statistics -----------------------------------------------------------------------------------------------------------------------
def moments(x, eps=LN_EPS):
    """(mean, rstd) per row, [rows, 2], in x's dtype."""
    mean = x.mean(1)
    return torch.stack((mean, 1.0 / torch.sqrt(x.var(1, unbiased=False) + eps)), 1)


def slice_moments(x, P):
    """Per column slice (mean, sum of squared deviations), [rows, P, 2]."""
    sl = x.view(x.shape[0], P, x.shape[1] // P)
    mu = sl.mean(2, keepdim=True)
    return torch.stack((mu[..., 0], ((sl - mu) ** 2).sum(2)), 2)


def stats_ref(rows_as_written, N, parts=0, eps=LN_EPS):
    """What a statistics-out launch must have written for the N values per row it stored: float64 (mean, rstd) [rows, 2], or `parts` per-slice
    (mean, M2) pairs [rows, parts, 2]."""
    x = rows_as_written[:, :N].double()
    return slice_moments(x, parts) if parts else moments(x, eps)


def _raw_moments_f32(x):
    """(mean, E[x^2] - E[x]^2) per row, every operation in float32: the single-pass form without a shift."""
    xf = x.float()
    m = xf.mean(1, keepdim=True)
    return m, ((xf * xf).mean(1, keepdim=True) - m * m).clamp(min=0.0)


def _stats_out(rows_as_written, mutant):
    """The forwarded (mean, rstd) of a residual-stream launch over the rows it wrote."""
    if mutant == "stats_unshifted":
        m, var = _raw_moments_f32(rows_as_written)
        return torch.cat((m, 1.0 / torch.sqrt(var + LN_EPS)), 1).to(rows_as_written.dtype)
    return moments(rows_as_written)


def _ln(x, gam, bet, dt, o, row, mutant):
    """LayerNorm of the f32 rows -> the 16-bit B fragments."""
    K = x.shape[1]
    mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    if mutant in ("chan_no_between_term", "chan_raw_moments"):
        p = o["stats_in"].to(x.dtype)
        if mutant == "chan_no_between_term":
            mean, var = p[..., 0].mean(1, keepdim=True), p[..., 1].sum(1, keepdim=True) / K
        else:
            mean = p[..., 0].sum(1, keepdim=True) / K
            var = (p[..., 1].sum(1, keepdim=True) / K - mean * mean).clamp(min=0)
    if mutant == "ln_var_n_minus_1":
        var = var * K / (K - 1)
    if mutant == "ln_var_raw_moments":
        mean, var = (t.to(x.dtype) for t in _raw_moments_f32(x))
    eps = 0.0 if mutant == "ln_no_eps" else LN_EPS
    return rT((x - mean) / torch.sqrt(var + eps) * gam.to(x.dtype) + bet.to(x.dtype), dt)


def _pair_bias(b, dt):
    hi = rT(b, dt)
    return hi, rT(b - hi, dt)


# ---- tok_linear / tok_linear_pool -----------------------------------------------------------------------------------------------------------------
def pool_tokens(B, H, W, mutant=None):
    """[B H W / 4, 4] source token of lane q of every 2 x 2 block, as tok_stream.hpp pool_token computes it."""
    hw2 = (H // 2) * (W // 2)
    prow = torch.arange(B * hw2)
    b, r = prow // hw2, prow % hw2
    w2 = (H // 2) if mutant == "pool_w_for_hw" else (W // 2)
    py, px = r // w2, r % w2
    q = torch.arange(4)
    dy, dx = (q >> 1) & 1, q & 1
    if mutant == "pool_dxdy_swapped":
        dy = dx
    tok = (b * 4 * hw2)[:, None] + (2 * py[:, None] + dy[None]) * W + 2 * px[:, None] + dx[None]
    return tok % (B * H * W)


def tok_linear_ref(row, o, dt, dtype=torch.float64, mutant=None):
    """One TOK_ROWS launch: dict(out = the whole output buffer [rows (pool: rows / 4), out_ld] in `dtype`, guard columns included,
    stats = what a statistics-out launch writes, or None).  dtype = float32 is chain32 (with the kernels' GELU form)."""
    assert mutant is None or mutant in TOK_MUTANTS, mutant
    K, N, out_ld, fmt = row["K"], row["N"], row["out_ld"], TOK_FORMAT[row["K"]]
    fast = dtype == torch.float32
    x = o["x"].to(dtype)
    if row["ln"] == 1:
        xn = _ln(x, o["gam"], o["bet"], dt, o, row, mutant)
    else:
        xn = rT(x, dt)                                       # ln = 2: f32 rows converted as they are; ln = 0: already 16-bit values
    nch = (N + 31) // 32
    w = torch.zeros(nch * 32, K, dtype=dtype)
    w[:N] = o["w"].to(dtype)
    bias = torch.zeros(nch * 32, dtype=dtype)
    if fmt == 32:
        hi, lo = _pair_bias(o["b"], dt)
        bias[:N] = hi.to(dtype) if mutant == "bias_hi_only" else hi.to(dtype) + lo.to(dtype)
    else:
        bias[:N] = o["b"].to(dtype)
    src = torch.arange(nch)                                  # the chunk whose weights chunk j is computed with
    slots = 4 if fmt == 32 else 3
    if mutant == "ring_stale_slot":
        src = torch.where(src >= slots, src - slots, src)
    ns = row["ns"] or 1
    if mutant == "split_ring_origin" and ns > 1:
        cps = -(-nch // ns)
        src = src - (src // cps) * cps
    idx = (src[:, None] * 32 + torch.arange(32)[None]).reshape(-1)
    y = (xn @ w[idx].t() + bias[idx])[:, :N]
    if row["gelu"]:
        y = _gelu(y, dt, fast)
    dst0 = o["dst0"].to(dtype)
    out = dst0.clone()
    if row["pool"]:
        B, H, W = row["grid"]
        quad = y[pool_tokens(B, H, W, mutant)]                # [prows, 4, N]
        out[:, :N] = quad.mean(1) if mutant == "pool_mean" else quad.max(1).values
    elif row["res"]:
        out[:, :N] = y if mutant == "res_overwrite" else dst0[:, :N] + y
    else:
        out[:, :N] = rT(y, dt)
    if mutant == "last_piece_dropped" and N % 32:
        piece = 8 if not (row["res"] or row["pool"]) and N % 8 == 0 and out_ld % 8 == 0 else 4
        out[:, N - piece:N] = dst0[:, N - piece:N]
    if mutant == "guard_written":
        out[:, N:min(32 * nch, out_ld)] = 0.0
    stats = None
    if row["stats_out"]:
        n = out_ld if mutant == "stats_over_ld" else N
        stats = slice_moments(out[:, :n], ns) if ns > 1 else moments(out[:, :n])
    return dict(out=out, stats=stats)


def tok_operands(row, dt):
    """Seeded operands of one TOK_ROWS row in dtype dt as CPU float32 tensors: x [rows, K] (16-bit values for ln = 0), w [N, K] (16-bit values), b
    f32, gam / bet, dst0 = the output buffer before the launch [rows | rows / 4, out_ld] (guards hold the sentinel, the residual form's N columns
    the old stream), stats_in.  Weights and bias are small enough that 16-bit outputs stay around or below 1.  LayerNorm rows come in five kinds within every
    launch: rows 0-31 sit 500 away from zero, rows 32-63 carry a ramp along K (slice means many sigma apart), rows 64-95 have a spread of 1e-3
    (variance near eps), rows 96-127 an outlier channel, the rest are plain."""
    g = _gen(row["id"], dt)
    K, N, rows = row["K"], row["N"], row["rows"]
    o = dict(w=rT(torch.randn(N, K, generator=g) * WSCALE / K ** 0.5, dt), b=torch.randn(N, generator=g) * 0.1,
             gam=torch.rand(K, generator=g) + 0.5, bet=torch.randn(K, generator=g) * 0.2, stats_in=None)
    if row["ln"] == 0:
        x = rT(torch.randn(rows, K, generator=g), dt)
    else:
        x = torch.randn(rows, K, generator=g) * 1.5 + 0.7
        if row["ln"] == 1:
            x[:32] += 500.0
            x[32:64] += torch.linspace(-20.0, 20.0, K)
            x[64:96] *= 1e-3
            x[96:128, 3] += 40.0
    o["x"] = x
    orows = rows // 4 if row["pool"] else rows
    f32out = row["res"] or row["pool"]
    dst0 = torch.full((orows, row["out_ld"]), SENT32 if f32out else SENT16)
    if row["res"]:
        dst0[:, :N] = torch.randn(orows, N, generator=g)
    o["dst0"] = dst0
    if row["stats_in"] == "pair":
        o["stats_in"] = moments(x.double()).float().contiguous()
    elif row["stats_in"]:
        o["stats_in"] = slice_moments(x.double(), row["stats_in"]).float().contiguous()
    return o


# ---- hiera_mlp --------------------------------------------------------------------------------------------------------------------------------------
def hiera_mlp_ref(row, o, dt, dtype=torch.float64, mutant=None):
    """x <- x + fc2(GELU(fc1(LayerNorm(x)))) on the first `rows` rows of the buffer [rows + 3, x_ld]: dict(out = the whole buffer, stats)."""
    assert mutant is None or mutant in MLP_MUTANTS + MLP_KIND_MUTANTS, mutant
    C, rows = row["C"], row["rows"]
    buf = o["x0"].to(dtype)
    upd = min(rows + 3, -(-rows // 128) * 128) if mutant == "mlp_rows_past_end" else rows
    x = buf[:upd, :C]
    out = buf.clone()
    out[:upd, :C] = x + _mlp_branch(x, row, o, dt, dtype, mutant)
    return dict(out=out, stats=_stats_out(out[:rows, :C], mutant) if row["stats_out"] else None)


def _mlp_branch(x, row, o, dt, dtype, mutant, k_order=None):
    """fc2(GELU(fc1(LayerNorm(x)))) + b2 in `dtype`: the LayerNorm output and the hidden activation are rounded to dt, fc1's bias is the packed
    hi + lo pair.  k_order: the channel order in which the normalised row meets fc1's columns (None: each its own)."""
    xn = _ln(x, o["gam"], o["bet"], dt, o, row, mutant)
    if k_order is not None:
        xn = xn[:, k_order]
    hi, lo = _pair_bias(o["b1"], dt)
    h = _gelu(xn @ o["w1"].to(dtype).t() + (hi.to(dtype) + lo.to(dtype)), dt, dtype == torch.float32)
    if mutant != "mlp_hidden_not_rounded":
        h = rT(h, dt)
    return h @ o["w2"].to(dtype).t() + o["b2"].to(dtype)


def row_kinds(x):
    """The five kinds of LayerNorm input on the leading rows of x [rows, C], in place, KIND_ROWS rows each (op_matrix.KIND_BLOCKS): 500 away from
    zero; a ramp along C; a spread of 1e-3 (variance near eps); an outlier in channel 0 -- the value the statistics hand-over shifts by -- and in
    the last channel.  The rest stay plain."""
    n, C = KIND_ROWS, x.shape[1]
    x[:n] += 500.0
    x[n:2 * n] += torch.linspace(-20.0, 20.0, C)
    x[2 * n:3 * n] *= 1e-3
    x[3 * n:4 * n, 0] += 40.0
    x[4 * n:5 * n, C - 1] += 40.0


def mlp_operands(row, dt):
    g = _gen(row["id"], dt)
    C, rows = row["C"], row["rows"]
    x0 = torch.full((rows + 3, row["x_ld"]), SENT32)
    x0[:, :C] = torch.randn(rows + 3, C, generator=g) * 1.5 + 0.3
    if row.get("kinds"):
        assert rows >= 6 * KIND_ROWS
        row_kinds(x0[:rows, :C])
    return dict(x0=x0, gam=torch.rand(C, generator=g) + 0.5, bet=torch.randn(C, generator=g) * 0.2,
                w1=rT(torch.randn(4 * C, C, generator=g) / C ** 0.5, dt), b1=torch.randn(4 * C, generator=g) * 0.3,
                w2=rT(torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5, dt), b2=torch.randn(C, generator=g) * 0.3)


# ---- proj_mlp (the proj form of cvmi_hiera_mlp) -----------------------------------------------------------------------------------------------
def proj_k_order(C):
    """proj_mlp.hpp: k index kappa of fc1's k-step stands for channel 8 ((kappa & 7) >> 2) + 4 (kappa >> 3) + (kappa & 3) of the step's 16."""
    n = torch.arange(C)
    k = n % 16
    return n - k + 8 * ((k & 7) >> 2) + 4 * (k >> 3) + (k & 3)


def proj_mlp_ref(row, o, dt, dtype=torch.float64, mutant=None):
    """x1 = x + ao Wp^T + bp;  x <- x1 + fc2(GELU(fc1(LayerNorm(x1)))) + b2 on the first `rows` rows of the buffer [rows + 3, x_ld]: dict(out =
    the whole buffer, stats).  ao and the weights arrive rounded to dt; x1 is never rounded."""
    assert mutant is None or mutant in PROJ_MUTANTS, mutant
    C, rows = row["C"], row["rows"]
    buf = o["x0"].to(dtype)
    upd = min(rows + 3, -(-rows // 128) * 128) if mutant == "proj_rows_past_end" else rows
    x = buf[:upd, :C]
    ao = o["ao"][torch.arange(upd).clamp(max=rows - 1)].to(dtype)          # (rows past the end: the kernel's clamped row)
    pj, bp = ao @ o["wp"].to(dtype).t(), o["bp"].to(dtype)
    x1 = x + (pj + (2.0 * bp if mutant == "proj_bias_twice" else bp))
    if mutant == "x1_through_16_bits":
        x1 = rT(x1, dt)
    ln_in = x + pj if mutant == "proj_bias_not_in_ln" else x if mutant == "ln_of_x_not_x1" else x1
    y = _mlp_branch(ln_in, row, o, dt, dtype, mutant, proj_k_order(C) if mutant == "fc1_k_natural_order" else None)
    out = buf.clone()
    out[:upd, :C] = (x + bp if mutant == "residual_drops_proj" else x1) + y
    stats = None
    if row["stats_out"]:
        stats = moments(x1[:rows]) if mutant == "stats_of_x1" else _stats_out(out[:rows, :C], mutant)
    return dict(out=out, stats=stats)


def proj_operands(row, dt):
    """Seeded operands of one PROJ_ROWS row: x0 = the f32 buffer before the launch [rows + 3, x_ld] (padding columns NaN), ao [rows, ao_ld]
    (16-bit values, padding NaN), wp / w1 / w2 (16-bit values), bp / b1 / b2 / gam / bet f32.  The row kinds are kinds of the LayerNorm's
    input x1: x1 is drawn (and, on a `kinds` row, shaped) first, then x = f32(x1 - (ao Wp^T + bp)) with the product in float64."""
    g = _gen(row["id"], dt)
    C, rows = row["C"], row["rows"]
    x1 = torch.randn(rows + 3, C, generator=g) * 1.5 + 0.3
    if row["kinds"]:
        assert rows >= 6 * KIND_ROWS
        row_kinds(x1[:rows])
    ao = torch.full((rows, row["ao_ld"]), float("nan"))
    ao[:, :C] = rT(torch.randn(rows, C, generator=g), dt)
    o = dict(ao=ao[:, :C], ao_buf=ao, wp=rT(torch.randn(C, C, generator=g) / C ** 0.5, dt), bp=torch.randn(C, generator=g) * 0.3,
             gam=torch.rand(C, generator=g) + 0.5, bet=torch.randn(C, generator=g) * 0.2,
             w1=rT(torch.randn(4 * C, C, generator=g) / C ** 0.5, dt), b1=torch.randn(4 * C, generator=g) * 0.3,
             w2=rT(torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5, dt), b2=torch.randn(C, generator=g) * 0.3)
    x1[:rows] = (x1[:rows].double() - (o["ao"].double() @ o["wp"].double().t() + o["bp"].double())).float()
    x0 = torch.full((rows + 3, row["x_ld"]), float("nan"))
    x0[:, :C] = x1
    o["x0"] = x0
    return o


# ---- rows -------------------------------------------------------------------------------------------------------------------------------------------
ALL_ROWS = {r["id"]: r for r in TOK_ROWS + MLP_ROWS + MLP_KIND_ROWS + PROJ_ROWS}


def operands(row, dt):
    return proj_operands(row, dt) if row.get("proj") else mlp_operands(row, dt) if "C" in row else tok_operands(row, dt)


def reference(row, o, dt, dtype=torch.float64, mutant=None):
    return (proj_mlp_ref if row.get("proj") else hiera_mlp_ref if "C" in row else tok_linear_ref)(row, o, dt, dtype, mutant)


@functools.lru_cache(maxsize=None)
def _row_case(rid, dt):
    row = ALL_ROWS[rid]
    o = operands(row, dt)
    return row, o, reference(row, o, dt)


def row_case(rid, dt):
    """(row, operands, fp64 reference) of a row in dtype dt: computed once per process, shared by every test, never modified."""
    return _row_case(rid, dt)


def _close(got, exp, tol):
    return float(((got.double() - exp.double()).abs() / (tol[1] + tol[0] * exp.double().abs())).max())


def _same(a, b):
    """Bit-equal float32 tensors (NaN padding compares equal to itself)."""
    return a.shape == b.shape and torch.equal(a.float().contiguous().view(torch.int32), b.float().contiguous().view(torch.int32))


def judge(row, dt, o, ref, out, stats=None, atol=None):
    """The matrix's verdict on one launch: `out` is the whole output buffer after it (float tensor, [.., out_ld] or the MLP's [rows + 3, x_ld]),
    `stats` what it wrote as statistics.  Returns (err / bound of the N (C) computed columns, largest |err|, list of failures)."""
    mlp = "C" in row
    n, nrows = (row["C"], row["rows"]) if mlp else (row["N"], out.shape[0])
    atol = ATOL[family(row), dt] if atol is None else atol
    r64 = ref["out"][:nrows, :n].double()
    err = (out[:nrows, :n].double() - r64).abs()
    ratio = float((err / (atol + RTOL[stored(row, dt)] * r64.abs())).max())
    fails = []
    if not ratio <= 1.0:
        fails.append(f"err/bound {ratio:.3f} (max|err| {float(err.max()):.3e}, {int((err / (atol + RTOL[stored(row, dt)] * r64.abs()) > 1).sum())} of {err.numel()} elements over)")
    before = o["x0"] if mlp else o["dst0"]
    if not _same(out[:, n:].float(), before[:, n:]):
        fails.append("guard columns behind the output were written")
    if mlp and not _same(out[nrows:].float(), before[nrows:]):
        fails.append("rows behind the last one were written")
    if row["stats_out"]:
        parts = 0 if mlp else (row["ns"] or 1)
        parts = parts if parts > 1 else 0
        exp = stats_ref(out[:nrows], n, parts)
        if stats is None or tuple(stats.shape) != tuple(exp.shape):
            fails.append("statistics missing or of the wrong shape")
        else:
            s = _close(stats, exp, STATS_PARTS_TOL if parts else STATS_PAIR_TOL)
            if not s <= 1.0:
                fails.append(f"forwarded statistics differ from the rows as written: err/bound {s:.3f}")
    return ratio, float(err.max()), fails


def measure(dts=("f16", "bf16")):
    """{(family, dtype): largest |chain32 - ref64| over the family's rows} and the same per (family, K, dtype)."""
    dev, per_k = {}, {}
    for rid, row in ALL_ROWS.items():
        for dt in dts:
            _, o, ref = row_case(rid, dt)
            c32 = reference(row, o, dt, torch.float32)
            n = row.get("N", row.get("C"))
            nrows = row["rows"] if "C" in row else c32["out"].shape[0]
            mx = float((c32["out"][:nrows, :n].double() - ref["out"][:nrows, :n]).abs().max())
            k = (family(row), dt)
            dev[k] = max(dev.get(k, 0.0), mx)
            kk = (family(row), row.get("K", row.get("C")), dt)
            per_k[kk] = max(per_k.get(kk, 0.0), mx)
    return dev, per_k


def measure_kinds(dts=("f16", "bf16")):
    """{(row id, dtype): largest |chain32 - ref64| per block of KIND_BLOCKS, then over the plain rows behind them} of every `kinds` row."""
    out = {}
    for rid, row in ALL_ROWS.items():
        if not row.get("kinds"):
            continue
        for dt in dts:
            _, o, ref = row_case(rid, dt)
            d = (reference(row, o, dt, torch.float32)["out"][:row["rows"], :row["C"]].double() - ref["out"][:row["rows"], :row["C"]]).abs().amax(1)
            nb = len(KIND_BLOCKS)
            out[rid, dt] = [float(d[KIND_ROWS * i:KIND_ROWS * (i + 1)].max()) for i in range(nb)] + [float(d[KIND_ROWS * nb:].max())]
    return out


def main():
    for (rid, dt), v in sorted(measure_kinds().items()):
        print("%-32s %-5s %s" % (rid, dt, "  ".join("%s %.3e" % kv for kv in zip(KIND_BLOCKS + ("plain",), v))))
    dev, per_k = measure()
    for k in sorted(dev):
        ks = "  ".join("K=%d %.3e" % (kk[1], v) for kk, v in sorted(per_k.items()) if (kk[0], kk[2]) == k)
        print("%-10s %-5s largest |chain32 - ref64| %.4e   constant %s   atol %s   [%s]" % (k[0], k[1], dev[k], CHAIN32_DEV.get(k), ATOL.get(k), ks))
    for dt in ("f16", "bf16"):
        e = gelu_form_error(dt)
        print("gelu_fast%s: max |err| %.3e; max relative error %.3e on 0.5 <= |x| <= 2, %.3e on 2^-6 <= |x|, x > -3" % ("_pk (fp16 arithmetic)" if dt == "f16" else " (f32 arithmetic)", *e))


if __name__ == "__main__":
    main()
