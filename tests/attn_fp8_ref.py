"""Reference side of the e4m3 AV-product rows (tests/op_matrix.py ATTN_FP8_ROWS): operands, the float64 emulation of the arithmetic
cvmi_attn_desc.av_fp8 states, the per-element bound derived from it, and deliberately wrong variants of the emulation (FP8_MUTANTS).
Importable without a GPU or the library.

The arithmetic (attention.hip: SOFTMAX_UPDATE72(P8_SUM_VALU), V_IMAGE_PIECE, PV8_STEP, NORMALISE_STORE), per 64-key tile:
    m    the running row maximum over the tiles so far (threshold 0: it moves whenever a tile exceeds it)
    x    = exp2(fma(s, c, -(m c - 8))) = p 2^8, c = f32(scale) * f32(log2 e) in f32; P = e4m3(x) (round to nearest even), block scale 2^-8
    V    = e4m3(clamp(v, +-448))
    O    <- O alpha + P V in f32, l <- l alpha + sum of the UNQUANTISED p, alpha = exp2(m_old c - m c);  o = O (1 / l), stored in the 16-bit type.

The bound.  Everything but the rounding of P is reproduced exactly or to f32 accuracy, so the kernel can leave the emulation by more than f32
noise only where ITS x lies on the other side of an e4m3 rounding boundary.  Its x differs from the emulation's by a relative delta:
    d_arg = c (e_s + e_m) + 2^-24 (2 |m c| + 8 + |arg|)       error of the exponent: the f32 dot product of dqk 16-bit terms, formed as the conv
                                                              matrix forms it, e_s = (dqk + 2) 2^-24 sum |q| |k|; e_m the same for the key
                                                              that holds the maximum (the row's largest e_s); the roundings of m c, m c - 8
                                                              and the fma
    delta = ln 2 d_arg + 2^-23                                v_exp_f32: 1 ulp.  The figure is the one AMD's ISA guides give for the f32
                                                              transcendentals (exp, log, rcp, rsq, sqrt: "1 ULP"); it is also what this
                                                              library's other bounds assume for v_exp_f32 / v_rcp_f32 (common.hpp, tests/detect_ref.py)
A key whose x lies within delta x of the midpoint of two neighbouring e4m3 values (the tie at 2^-10 between 0 and the smallest subnormal 2^-9
included) may round the other way and moves the output by that step:
    bound = sum_{k near a midpoint} step_e4m3(x_k) 2^-8 |V_k| / l                 (1) a flipped P
          + (Nk + 2 T + 2) 2^-23 sum_k P_k |V_k| / l                              (2) f32 accumulation of Nk products (exact each: two e4m3 values) and
                                                                                      T = Nk / 64 rescales; 2^-23, not 2^-24, per step: the matrix
                                                                                      pipe's adder is not specified to round to nearest
          + |o| (sum_k delta_k p_k / l + (Nk + 2 T) 2^-24)                        (3) l: sums the kernel's own p (each off by delta) in f32
          + 3 2^-24 |o|                                                           (4) the epilogue, counted from NORMALISE_STORE: 1 / l (at most
                                                                                      1 ulp = 2 half-ulps, whether a division or v_rcp_f32) and one product
          + max(u |o|, tiny)                                                      (5) half an ulp of the stored type (u = 2^-11 / 2^-8; tiny = half
                                                                                      the subnormal spacing, 2^-25 in fp16)
With exact_scores (integer q and k: every partial sum of the dot product is an integer below 2^24) e_s = e_m = 0.
Term (2) is the one assumption about hardware the bound makes: that the block-scaled matrix instruction adds its 64 products and the accumulator
with no more than one f32 step of error each.  On an MI355X a few elements per case leave the bound by a factor of up to 1.4 (random) and 5.8
(exact), and in the exact kind each of them is one product, 2^-11 to 2^-12 of the largest of its 16-key operand group, missing from the sum: the assumption
does not hold as stated.  The bound is kept as derived; tests/test_attention_fp8_matrix_gpu.py RELAX lists the rows and their measured ratios.

Operand kinds (operands()):
    random   q, k ~ N(0, 1), v ~ 1.7 N(0, 1), five V elements beyond +-448 (the clamp); scale dqk^-1/2.  q_log2 rows: q carries scale * log2(e).
    exact    q in {-2..2}, k in {-1, 0, 1}, descriptor scale ln 2 (c = 1 exactly, checked) or q_log2 = 1: every score is an integer in log2 units, every
             p a power of two, x exact in e4m3 down to 2^-9; V from e4m3 values: mostly {0, +-2^-9, +-2^-6, +-1/8, +-1/4}, one in 32 is +-448.  The
             only key on a rounding boundary is the tie at gap 18 (x = 2^-10); the expected output is known to f32 and the output's rounding."""
import functools
import zlib

import torch

LN2, LOG2E = 0.6931471805599453, 1.4426950408889634
TORCH_T = {"f16": torch.float16, "bf16": torch.bfloat16}
UNIT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
TINY = {"f16": 2.0 ** -25, "bf16": 2.0 ** -134}
KINDS = ("random", "exact")
V_CLAMPED = 5                                        # random kind: V elements beyond +-448
FP8_MUTANTS = ("l_of_quantised_p", "p_scale_2^7", "p_truncated", "v_unclamped_saturates", "key_halves_swapped", "d_tiles_swapped", "tile_32")


def _fp8_av_emulation(q, k, v, scale, tile=64):
    """The arithmetic cvmi_attn_desc.av_fp8 states, tile by tile as the kernels run it: per 64-key tile the running row maximum m, P = e4m3(exp(s - m)
    * 2^8) / 2^8, V = e4m3(clamp(v, +-448)), O <- O * exp(m_old - m) + P V in fp32, row sums of the UNquantised p.  [.., Nq, d] x [.., Nk, d]."""
    f8 = lambda t: t.to(torch.float8_e4m3fn).float()
    s = (q @ k.transpose(-1, -2)) * scale
    Nk = k.shape[-2]
    m = torch.full(s.shape[:-1] + (1,), float("-inf"))
    o = torch.zeros(q.shape[:-1] + (v.shape[-1],))
    l = torch.zeros_like(m)
    v8 = f8(v.clamp(-448, 448))
    for k0 in range(0, Nk, tile):
        st = s[..., k0:k0 + tile]
        m_new = torch.maximum(m, st.amax(-1, keepdim=True))
        alpha = torch.exp(m - m_new)
        pt = torch.exp(st - m_new)
        o = o * alpha + (f8(pt * 256.0) / 256.0) @ v8[..., k0:k0 + tile, :]
        l = l * alpha + pt.sum(-1, keepdim=True)
        m = m_new
    return o / l


def c_log2(scale, q_log2=0):
    """The kernel's c: log2 units per unit of q.k, as cvmi_attention and the kernels form it in f32 (q_log2: the descriptor's scale is replaced by ln 2)."""
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    return float(f32(LN2 if q_log2 else scale) * f32(1.44269504088896340736))


def _f8(x):
    """Round to nearest even onto e4m3 (float64 in and out; the values given here are exact in f32 or far from a midpoint in it)."""
    return x.float().to(torch.float8_e4m3fn).double()


def _f8_trunc(x):
    """Round toward zero onto e4m3, x >= 0."""
    step = torch.exp2(torch.floor(torch.log2(x.clamp(min=2.0 ** -40))).clamp(min=-6.0) - 3.0)
    return torch.floor(x / step) * step


def _step_and_mid(x):
    """x > 0 (float64) -> (spacing of the e4m3 values around x, the midpoint of x's two neighbours)."""
    step = torch.exp2(torch.floor(torch.log2(x.clamp(min=2.0 ** -40))).clamp(min=-6.0) - 3.0)
    lo = torch.floor(x / step) * step
    return step, lo + 0.5 * step


def fp8_av_emulation(q, k, v, c, out="f16", exact_scores=False, mutant=None, parts=False):
    """(o, bound) of the module's docstring in float64; q [.., Nq, dqk], k [.., Nk, dqk], v [.., Nk, dv] hold 16-bit values, c = c_log2(...).
    mutant: one of FP8_MUTANTS (the bound returned is still the true arithmetic's formula on the mutant's numbers: use the true call's).
    parts: return term (1) of the bound in place of the bound."""
    assert mutant is None or mutant in FP8_MUTANTS, mutant
    q, k, v = q.double(), k.double(), v.double()
    Nk, dqk = k.shape[-2], k.shape[-1]
    tile = 32 if mutant == "tile_32" else 64
    pscale = 7.0 if mutant == "p_scale_2^7" else 8.0
    s = q @ k.transpose(-1, -2)
    es = torch.zeros_like(s) if exact_scores else (dqk + 2) * 2.0 ** -24 * (q.abs() @ k.abs().transpose(-1, -2))
    em = es.amax(-1, keepdim=True)
    if mutant == "v_unclamped_saturates":                       # no clamp: the conversion's overflow result (NaN) reaches the product
        v8 = torch.where(v.abs() > 448, torch.full_like(v, float("nan")), _f8(v.clamp(-448, 448)))
    else:
        v8 = _f8(v.clamp(-448, 448))
    if mutant == "d_tiles_swapped":
        v8 = torch.cat((v8[..., 32:64], v8[..., :32], v8[..., 64:]), -1)
    if mutant == "key_halves_swapped":
        v8 = v8.reshape(v8.shape[:-2] + (Nk // 64, 2, 32, v8.shape[-1])).flip(-3).reshape(v8.shape)
    m = torch.full(s.shape[:-1] + (1,), float("-inf"), dtype=torch.float64)
    o = torch.zeros(q.shape[:-1] + (v.shape[-1],), dtype=torch.float64)
    flip, absacc, l, ldel = torch.zeros_like(o), torch.zeros_like(o), torch.zeros_like(m), torch.zeros_like(m)
    for k0 in range(0, Nk, tile):
        st, vt = s[..., k0:k0 + tile], v8[..., k0:k0 + tile, :]
        m_new = torch.maximum(m, st.amax(-1, keepdim=True))
        alpha = torch.exp2((m - m_new) * c)
        arg = (st - m_new) * c + pscale
        x = torch.exp2(arg)
        delta = LN2 * (c * (es[..., k0:k0 + tile] + em) + 2.0 ** -24 * (2 * (m_new * c).abs() + 8 + arg.abs())) + 2.0 ** -23
        step, mid = _step_and_mid(x)
        near = ((x - mid).abs() <= delta * x).double()
        P = (_f8_trunc(x) if mutant == "p_truncated" else _f8(x)) * 2.0 ** -pscale
        p = x * 2.0 ** -pscale
        o = o * alpha + P @ vt
        flip = flip * alpha + (near * step * 2.0 ** -pscale) @ vt.abs()
        absacc = absacc * alpha + P @ vt.abs()
        l = l * alpha + (P if mutant == "l_of_quantised_p" else p).sum(-1, keepdim=True)
        ldel = ldel * alpha + (delta * p).sum(-1, keepdim=True)
        m = m_new
    T = Nk // 64
    o = o / l
    bound = (flip / l + (Nk + 2 * T + 2) * 2.0 ** -23 * absacc / l + o.abs() * (ldel / l + (Nk + 2 * T) * 2.0 ** -24) + 3 * 2.0 ** -24 * o.abs()
             + torch.clamp(UNIT[out] * o.abs(), min=TINY[out]))
    return o, (flip / l if parts else bound)


def _seed(row, dt, kind):
    return zlib.crc32(f"{row['id']}|{dt}|{kind}".encode())


def operands(row, dt, kind):
    """(q, k, v, scale, exact_scores) of a row of op_matrix.ATTN_FP8_ROWS: f32 tensors [B, heads, N, 72] already rounded to dt (window rows: B =
    the window count, N = win^2), and the scale the descriptor carries (q_log2 rows: 123, which the library must ignore)."""
    assert kind in KINDS and not row.get("q_pool"), (row["id"], kind)
    B, H, Nq, Nk, dqk, dv = (row[x] for x in ("B", "heads", "Nq", "Nk", "dqk", "dv"))
    g = torch.Generator().manual_seed(_seed(row, dt, kind))
    rnd = lambda t: t.to(TORCH_T[dt]).float()
    if kind == "random":
        scale = dqk ** -0.5
        q, k, v = (torch.randn(B, H, n, d, generator=g) for n, d in ((Nq, dqk), (Nk, dqk), (Nk, dv)))
        v *= 1.7
        at = torch.randperm(v.numel(), generator=g)[:V_CLAMPED]
        v.view(-1)[at] = torch.tensor([600.0, -600.0, 450.0, -3000.0, 60000.0])[:V_CLAMPED]
        if row["q_log2"]:
            q *= scale * LOG2E
        return rnd(q), rnd(k), rnd(v), (123.0 if row["q_log2"] else scale), False
    q = torch.randint(-2, 3, (B, H, Nq, dqk), generator=g).float()
    k = torch.randint(-1, 2, (B, H, Nk, dqk), generator=g).float()
    small = torch.tensor([0.0, 0.0, 2.0 ** -9, -2.0 ** -9, 2.0 ** -6, -2.0 ** -6, 0.125, -0.125, 0.25, -0.25])
    v = small[torch.randint(0, len(small), (B, H, Nk, dv), generator=g)]
    big = torch.randint(0, 64, (B, H, Nk, dv), generator=g)
    v = torch.where(big == 0, torch.tensor(448.0), torch.where(big == 1, torch.tensor(-448.0), v))
    assert torch.equal(rnd(v), v) and torch.equal(rnd(q), q)
    return q, k, v, (123.0 if row["q_log2"] else LN2), True


@functools.lru_cache(maxsize=4)
def case(rid, dt, kind):
    """(row, q, k, v, scale, c, emulation, bound) of one row, type and operand kind: computed once, shared, never modified."""
    from op_matrix import ATTN_FP8_ROWS
    row = next(r for r in ATTN_FP8_ROWS if r["id"] == rid)
    q, k, v, scale, exact = operands(row, dt, kind)
    c = c_log2(scale, row["q_log2"])
    emu, bound = fp8_av_emulation(q, k, v, c, out=dt, exact_scores=exact)
    return row, q, k, v, scale, c, emu, bound


def score_gaps(q, k):
    """Integer gaps m - s of the exact kind per 64-key tile against the running maximum, as a flat int64 tensor (asserts integrality)."""
    s = q.double() @ k.double().transpose(-1, -2)
    assert torch.equal(s, s.round())
    m = torch.cummax(s.reshape(s.shape[:-1] + (-1, 64)).amax(-1), -1).values                  # running maximum after each tile
    return (m.unsqueeze(-1) - s.reshape(s.shape[:-1] + (-1, 64))).reshape(-1).long()
