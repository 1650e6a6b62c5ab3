"""Case rows of the proj + MLP launch (csrc/proj_mlp.hpp, the proj form of cvmi_hiera_mlp_stats): one row per (instance, row count).  `expect` is
the tag cvmi_last_kernel() reports.  Row counts: 5 = less than one wave's 32-token tile; 1000 and 128 * 3 + 37 (C = 144) / 777 (C = 288) end in a
ragged 128-row workgroup and run more than one workgroup.  tests/test_proj_mlp_cpu.py checks that every instance the header can launch has a
row here; tests/test_proj_mlp_gpu.py runs the rows in fp16 and bf16."""

PROJ_MLP_ROWS = [
    dict(id="c144_rows5", C=144, rows=5, expect="proj_mlp_kernel<144, 1>"),
    dict(id="c144_rows1000", C=144, rows=1000, expect="proj_mlp_kernel<144, 1>"),
    dict(id="c144_rows421", C=144, rows=128 * 3 + 37, expect="proj_mlp_kernel<144, 1>"),
    dict(id="c288_rows5", C=288, rows=5, expect="proj_mlp_kernel<288, 2>"),
    dict(id="c288_rows777", C=288, rows=777, expect="proj_mlp_kernel<288, 2>"),
]
