"""CPU guard of the token path's C ABI (include/cvmi355.h: cvmi_tok_desc / cvmi_mlp_desc): what cvmi_tok_linear and cvmi_hiera_mlp refuse on the
host, before any launch.  No GPU is needed: every refusal is decided from the descriptor alone and the addresses are never dereferenced.
  - ln_stats_out_parts: the caller states the layout it allocated ln_stats_out for; a launch that would write another one is refused
  - LayerNorm input + residual output on overlapping memory, in a launch whose workgroups share row blocks, is refused
  - every scalar field lands where its name says: the refusal that echoes a value echoes the one that was set."""
import ctypes
import os

import pytest

from circuitvision_amd import _lib
from circuitvision_amd._lib import ACT_NONE, BF16, F16, F32

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libcvmi355.so not built")

A = 1 << 32                                                  # an aligned, never-dereferenced address
FAR = 1 << 40                                                # ... and one far behind every range that starts at A


def tok(**kw):
    """A valid K = N = 144 LayerNorm -> 16-bit launch on 256 rows, with the fields of kw set over it."""
    f = dict(gamma=A, beta=A, w_packed=A, out=FAR, rows=256, in_ld=144, in_f32_layernorm=1, out_ld=144, K=144, N=144, act=ACT_NONE, dtype=F16,
             eps=1e-6, **{"in": A})
    f.update(kw)
    return _lib.TokDesc(**f)


def mlp(**kw):
    f = dict(x=A, gamma=A, beta=A, w_packed=A, b2=A, rows=256, x_ld=144, C=144, dtype=F16, eps=1e-6)
    f.update(kw)
    return _lib.MlpDesc(**f)


def refused(d, match):
    fn = _lib.load().cvmi_tok_linear if isinstance(d, _lib.TokDesc) else _lib.load().cvmi_hiera_mlp
    rc = fn(ctypes.byref(d), None)
    assert rc != 0, match
    with pytest.raises(_lib.CvmiError, match=match):
        _lib.check(rc, "refusal")


NOT_ALIGNED = r"tok_linear: pointers / ld not aligned"      # the later, deliberate refusal of a call that got past the check under test


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_ln_stats_out_comes_in_the_layout_the_caller_allocated(dtype):
    lib = _lib.load()
    P = lib.cvmi_tok_linear_stats_parts(2048, 576, 576)      # row blocks shared by P workgroups: float[rows][P][2]
    assert P > 1
    res576 = dict(rows=2048, K=576, N=576, in_ld=576, out_ld=576, out_f32_residual=1, ln_stats_out=A, ln_stats_eps=1e-6, dtype=dtype)
    refused(tok(**res576, ln_stats_out_parts=0), rf"ln_stats_out_parts=0, but this launch writes ln_stats_out in {P} parts")
    refused(tok(**res576, ln_stats_out_parts=P + 1), rf"ln_stats_out_parts={P + 1}, but this launch writes ln_stats_out in {P} parts")
    refused(tok(**res576, ln_stats_out_parts=P, out=FAR + 4), NOT_ALIGNED)           # the right P passes that check
    refused(tok(**{**res576, "ln_stats_out": None}, ln_stats_out_parts=0, out=FAR + 4), NOT_ALIGNED)       # no statistics out: nothing to state
    assert lib.cvmi_tok_linear_stats_parts(65536, 576, 576) == 0                       # one workgroup per row block: pairs
    refused(tok(**{**res576, "rows": 65536}, ln_stats_out_parts=P), rf"ln_stats_out_parts={P}, but this launch writes ln_stats_out in 0 parts")
    refused(tok(**{**res576, "rows": 65536}, ln_stats_out_parts=0, out=FAR + 4), NOT_ALIGNED)
    # the other formats never share row blocks
    assert lib.cvmi_tok_linear_stats_parts(2048, 144, 144) == 0
    res144 = dict(rows=2048, out_f32_residual=1, ln_stats_out=A, dtype=dtype)
    refused(tok(**res144, ln_stats_out_parts=P), rf"ln_stats_out_parts={P}, but this launch writes ln_stats_out in 0 parts")
    refused(tok(**res144, ln_stats_out_parts=0, out=FAR + 4), NOT_ALIGNED)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_layernorm_input_may_not_alias_the_residual_output_where_row_blocks_are_shared(dtype):
    OVERLAP = r"LayerNorm input and residual output overlap"
    shape = dict(K=576, N=576, in_ld=576, out_ld=576, out_f32_residual=1, dtype=dtype)
    size = 2048 * 576 * 4                                    # bytes of [in, in + rows * in_ld * 4)
    assert _lib.load().cvmi_tok_linear_stats_parts(2048, 576, 576) > 1
    refused(tok(**shape, rows=2048, out=A), OVERLAP)                                   # in place
    refused(tok(**shape, rows=2048, out=A + size - 16), OVERLAP)                       # the last 16 bytes
    refused(tok(**shape, rows=2048, out=A - size + 16), OVERLAP)                       # ... and the first
    refused(tok(**shape, rows=2048, out=A, ln_stats_out=A, ln_stats_out_parts=_lib.load().cvmi_tok_linear_stats_parts(2048, 576, 576)), OVERLAP)
    refused(tok(**shape, rows=2048, out=A + size, gamma=A + 4), NOT_ALIGNED)           # back to back: no overlap
    refused(tok(**shape, rows=2048, out=A - size, gamma=A + 4), NOT_ALIGNED)
    # 256 * 256 rows fill the chip with one workgroup per row block: nothing is shared, the same pointers pass the check
    refused(tok(**shape, rows=256 * 256, out=A, gamma=A + 4), NOT_ALIGNED)
    # ... as do the forms that cannot race: a 16-bit input, or a K whose row blocks are never shared
    refused(tok(**shape, in_f32_layernorm=0, rows=2048, out=A, w_packed=A + 4), NOT_ALIGNED)
    refused(tok(rows=2048, out_f32_residual=1, out=A, gamma=A + 4, dtype=dtype), NOT_ALIGNED)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_scalar_fields_land_where_they_are_named(dtype):
    refused(tok(dtype=dtype, K=145), r"tok_linear: K=145 is not built")
    refused(tok(dtype=dtype, in_ld=143), r"not aligned \(in_ld=143 out_ld=144 N=144\)")
    refused(tok(dtype=dtype, out_ld=142), r"not aligned \(in_ld=144 out_ld=142 N=144\)")
    refused(tok(dtype=dtype, N=146, out_ld=148), r"not aligned \(in_ld=144 out_ld=148 N=146\)")
    refused(tok(dtype=dtype, rows=255), r"rows must be a multiple of 256")
    refused(tok(dtype=dtype, in_f32_layernorm=3), r"in_f32_layernorm must be 0, 1 or 2")
    refused(tok(dtype=dtype, out_f32_residual=1, act=_lib.ACT_GELU), r"act must be NONE, or GELU with 16-bit output")
    refused(tok(dtype=dtype, ln_stats_in=A, ln_stats_in_parts=65), r"ln_stats_in_parts out of range")
    refused(tok(dtype=dtype, in_f32_layernorm=0, ln_stats_in=A), r"ln_stats_in needs the LayerNorm input form")
    refused(tok(dtype=dtype, K=576, in_ld=576, in_f32_layernorm=2), r"K = 144 and 288")
    # the pool form is selected by the token grid
    pool = dict(dtype=dtype, rows=512, pool_h=16, pool_w=16)
    refused(tok(**{**pool, "pool_w": 15}), r"tok_linear_pool: bad arguments")
    refused(tok(**{**pool, "rows": 768, "pool_w": 32}), r"tok_linear_pool: bad arguments")       # no whole number of 16 x 32 grids
    refused(tok(**pool, K=160), r"tok_linear_pool: K=160 is not built")
    refused(tok(**pool, in_ld=146), r"tok_linear_pool: pointers / ld not aligned \(in_ld=146 out_ld=144 N=144\)")
    refused(tok(**pool, out_f32_residual=1), r"tok_linear_pool: the pool form takes")
    refused(mlp(dtype=dtype, C=160, x_ld=160), r"hiera_mlp: C=160 is not built")
    refused(mlp(dtype=dtype, x_ld=142), r"hiera_mlp: pointers / ld must be 16-byte aligned")
    refused(mlp(dtype=dtype, rows=0), r"hiera_mlp: bad arguments")
    refused(mlp(dtype=dtype, ao=A, bp=A, ao_ld=136), r"proj_mlp: ao_ld=136 must be")
    if dtype == F16:
        refused(tok(dtype=F32), r"tok_linear: dtype must be")
        refused(tok(dtype=F32, pool_h=16, pool_w=16), r"tok_linear_pool: dtype must be")
        refused(mlp(dtype=F32), r"hiera_mlp: dtype must be")
