"""CPU guard on the per-op GPU coverage (tests/op_matrix.py): every dual-built entry point has a bf16 test, every attention kernel family the
dispatcher can launch has a row in the dispatch matrix.  Adding an entry point or a kernel without its per-op test fails here, on any checkout."""
import ast
import glob
import os
import re

from op_matrix import ATTN_ROWS, BF16_OPS, SHARE_ROWS

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "circuitvision_amd", "csrc")


def dual_built_entries(csrc=CSRC):
    """Names wrapped in CVMI_ENTRY(...) anywhere in the library's HIP sources: the entry points compiled once per 16-bit operand type."""
    names = set()
    for path in glob.glob(os.path.join(csrc, "*.hip")):
        names.update(re.findall(r"CVMI_ENTRY\((cvmi_\w+)\)", open(path).read()))
    return names


def attention_families(csrc=CSRC):
    """Kernel families attention.hip tags before a launch: the identifier in front of the template arguments of each cvmi_note_kernel("...")."""
    src = open(os.path.join(csrc, "attention.hip")).read()
    return {re.match(r"\s*(\w+)", s).group(1) for s in re.findall(r'cvmi_note_kernel\(\s*"([^"]*)"', src)}


def stray_getenv(sources):
    """(file, line) of every getenv in {file name: text} other than the two the library keeps: hiera_mlp.hip's per-call read of the
    CVMI_MLP_PIPE test hook, and reads inside `#ifdef CVMI_MLP_DIAGS` (a timing-only build that never reaches the shipped library)."""
    hits = []
    for name, text in sorted(sources.items()):
        diag_depth = 0                                  # > 0: inside #ifdef CVMI_MLP_DIAGS (counting the #if blocks nested in it)
        for no, line in enumerate(text.splitlines(), 1):
            directive = line.strip()
            if diag_depth:
                if directive.startswith("#if"):
                    diag_depth += 1
                elif directive.startswith("#endif"):
                    diag_depth -= 1
                continue
            if directive == "#ifdef CVMI_MLP_DIAGS":
                diag_depth = 1
                continue
            for m in re.finditer(r"getenv\s*\(([^)]*)\)", line):
                if not (name == "hiera_mlp.hip" and m.group(1).strip() == '"CVMI_MLP_PIPE"'):
                    hits.append((name, no))
    return hits


def _test_functions(module):
    tree = ast.parse(open(os.path.join(HERE, module)).read())
    return {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}


def missing_bf16_tests(entries, table=BF16_OPS):
    """[(entry, why)] for entry points without a usable row in the bf16 table."""
    out = []
    for e in sorted(entries):
        if e not in table:
            out.append((e, "no row in op_matrix.BF16_OPS"))
            continue
        module, fn = table[e]
        funcs = _test_functions(module)
        if fn not in funcs:
            out.append((e, f"{module} has no function {fn}"))
        elif module not in ("test_bf16_ops_gpu.py", "test_attention_matrix_gpu.py") and "BF16" not in ast.get_source_segment(open(os.path.join(HERE, module)).read(), funcs[fn]) \
                and not any("BF16" in ast.unparse(d) for d in funcs[fn].decorator_list):
            out.append((e, f"{module}::{fn} does not run BF16"))
    return out


def test_every_dual_built_entry_point_has_a_bf16_test():
    entries = dual_built_entries()
    assert len(entries) >= 15, sorted(entries)                 # the parser still finds the entry points
    assert not missing_bf16_tests(entries), missing_bf16_tests(entries)
    stale = set(BF16_OPS) - entries
    assert not stale, f"op_matrix.BF16_OPS names entry points that no longer exist: {sorted(stale)}"


def test_a_new_entry_point_without_a_test_is_caught():
    entries = dual_built_entries() | {"cvmi_x"}
    assert [e for e, _ in missing_bf16_tests(entries)] == ["cvmi_x"]
    table = dict(BF16_OPS)
    table.pop("cvmi_cast")
    assert [e for e, _ in missing_bf16_tests(dual_built_entries(), table)] == ["cvmi_cast"]


def test_every_attention_kernel_family_is_in_the_dispatch_matrix():
    fams = attention_families()
    assert {"attn_f32_kernel", "attn64_kernel", "attn_f16_kernel"} <= fams, fams        # the parser still finds the launches
    tags = {r["expect"] for r in ATTN_ROWS} | {s[-1] for s in SHARE_ROWS}
    covered = {re.match(r"(\w+)", t).group(1) for t in tags}
    assert fams <= covered, f"attention kernel families with no row in op_matrix.ATTN_ROWS: {sorted(fams - covered)}"
    assert covered <= fams, f"op_matrix.ATTN_ROWS expects kernels attention.hip no longer launches: {sorted(covered - fams)}"


def test_matrix_rows_are_well_formed():
    ids = [r["id"] for r in ATTN_ROWS]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    for r in ATTN_ROWS:
        assert set(r["dtypes"]) <= {"f16", "bf16", "f32"} and r["dtypes"], r["id"]
        assert r["layout"] in ("sep", "qkv", "kv256", "grid"), r["id"]
        assert r["layout"] != "qkv" or r["Nq"] == r["Nk"], r["id"]
        if r["win"]:
            assert r["gh"] % r["win"] == 0 and r["gw"] % r["win"] == 0 and r["Nk"] == r["win"] ** 2, r["id"]
        if r["dtypes"] != ("f32",):
            assert r["dqk"] % 8 == 0 and r["dv"] % 8 == 0 and r["o_pad"] % 8 == 0, r["id"]      # the 16-bit kernels' alignment contract


def test_the_native_library_reads_no_tuning_switch():
    """Dispatch depends on shapes alone: a getenv in the HIP sources would bring back a run-time A/B switch (and the kernel variants only it
    reaches, shipped untested).  A/B runs load a second build through CVMI_LIB_PATH instead."""
    sources = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))}
    assert "getenv(\"CVMI_MLP_PIPE\")" in sources["hiera_mlp.hip"]          # the scan sees the one allowed read
    assert stray_getenv(sources) == [], stray_getenv(sources)
    probe = {"x.hip": 'int a = atoi(getenv("CVMI_X"));\n#ifdef CVMI_MLP_DIAGS\n#if 1\n#endif\ngetenv("D");\n#endif\ngetenv ("Y");\n',
             "hiera_mlp.hip": 'getenv("CVMI_MLP_PIPE"); getenv("CVMI_MLP_VAR");\n'}
    assert stray_getenv(probe) == [("hiera_mlp.hip", 1), ("x.hip", 1), ("x.hip", 7)]
