"""Case rows of the proj + MLP launch (csrc/proj_mlp.hpp, the proj form of cvmi_hiera_mlp) that tests/test_proj_mlp_gpu.py runs against its
own fp64 statement and the two launches: the five (instance, row count) pairs of op_matrix.PROJ_TODAY, derived from op_matrix.PROJ_ROWS -- the
table the token-path matrix (tests/test_tok_matrix_gpu.py) runs at every wave and workgroup edge -- and re-exported here with it.  `expect` is
the tag cvmi_last_kernel() reports.  Row counts: 5 = less than one wave's 32-token tile; 1000 and 128 * 3 + 37 (C = 144) / 777 (C = 288) end in a
ragged 128-row workgroup and run more than one workgroup.  tests/test_proj_mlp_cpu.py checks that every instance the header can launch has a
row here."""
from op_matrix import PROJ_ROWS, PROJ_TODAY

PROJ_MLP_ROWS = [dict(id="c%d_rows%d" % (r["C"], r["rows"]), C=r["C"], rows=r["rows"], expect=r["expect"])
                 for C, rows in PROJ_TODAY for r in PROJ_ROWS
                 if (r["C"], r["rows"]) == (C, rows) and r["stats_out"] and not r["kinds"] and r["x_ld"] == C + 4 and r["ao_ld"] == C + 8]
