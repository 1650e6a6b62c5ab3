"""CPU guard on the per-op GPU coverage (tests/op_matrix.py): every dual-built entry point has a bf16 test, every attention kernel family the
dispatcher can launch has a row in the dispatch matrix, every template instance of its two head-dim-72 launchers (launch_res256, launch_dma72:
the e4m3 AV-product instances among them, ATTN_FP8_ROWS) is some row's expected tag, and so has every kernel family and template instance of cvmi_conv2d's dispatcher
(CONV_ROWS), every built instance of the three fused YOLO11 kernels (FUSED_ROWS), and every layernorm_kernel instance, SPPF kernel and
refinement kernel of the helper dispatchers (LN_ROWS, HELPER_ROWS), every branch combination and edge of the detector's tail (NMS_ROWS,
DECODE_ROWS), and every instance of the token-stationary kernels with the chunk counts,
split counts, pool grids and statistics forms their rings and index arithmetic need (TOK_ROWS, MLP_ROWS), and every entry point and output-type
instance of the resampling kernels with the constants their rows were built from (RESAMPLE_ROWS), and every trace path, LDS threshold and
launch-table edge of the contour stage (CONTOUR_ROWS, PREPARE_ROWS).  Adding an entry point or a kernel
without its per-op test fails here, on any checkout."""
import ast
import glob
import os
import re

from op_matrix import (ATTN_FP8_FALLBACK_ROWS, ATTN_FP8_ROWS, ATTN_ROWS, BF16_OPS, C3K2_INSTANCES, CONV_ROWS, DECODE_NC_MAX, DECODE_REFUSED, DECODE_ROWS, FUSED_MUTANT_ROWS, NMS_A_EDGES, NMS_CAND_BYTES,
                       NMS_KINDS, NMS_LDS_A, NMS_MAX_A, NMS_MAX_DET, NMS_MAX_NMS, NMS_N_EDGES, NMS_NTHR_N, NMS_REFUSED, NMS_ROWS, NMS_WS_RECORD, decode_tag, nms_pick,
                       nms_tag, nms_workspace, FUSED_ROWS, HELPER_ROWS, LN_DUAL_ROWS, LN_FORMS, LN_NCAND, LN_ROWS,
                       MLP_INSTANCES, MLP_ROWS, SHARE_ROWS, SPPF_LDS_PIXELS, TNAME, TOK_FORMAT, TOK_INSTANCES, TOK_KS, TOK_MUTANT_ROWS, TOK_NCH, TOK_NCH_FAMILIES,
                       TOK_PARTS, TOK_ROWS, TOK_SLOTS, TOK_SPLIT_TABLE, TOK_UNSEEN_MUTANTS, c3k2_max_wgs_per_cu, c3k2_tag, conv_expect, ln_pick, ln_reachable,
                       ln_tag, mlp_pick, tl16_splits, tok_dispatch, tok_nch_family, tok_pick)
from op_matrix import KIND_BLOCKS, KIND_ROWS, MLP_KIND_ROWS, MLP_ROW_COUNTS, PROJ_INSTANCES, PROJ_ROWS, PROJ_TODAY, proj_pick
from op_matrix import AA_MAXTAPS, MASK_ENTRY, RECT_MAX, RESAMPLE_GRID_CAP, RESAMPLE_ROWS, TRANSFORM_ENTRY
from op_matrix import (BALLOT_LANES, CONTOUR_CAPACITY_ROW, CONTOUR_GRID_CAP, CONTOUR_ROWS, PLANE_MAX, PREPARE_ROWS, ROOT_ROWS_PER_BLOCK, TRACE_LANES, TRACE_LDS_MAX,
                       TRACE_LDS_OPTIN, contour_tag, plane_shape, trace_lds_bytes)

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
    """(file, line) of every getenv in {file name: text} other than the one the library keeps: hiera_mlp.hip's per-call read of the
    CVMI_MLP_PIPE test hook.  No preprocessor block is exempt."""
    hits = []
    for name, text in sorted(sources.items()):
        for no, line in enumerate(text.splitlines(), 1):
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
        elif module not in ("test_bf16_ops_gpu.py", "test_attention_matrix_gpu.py", "test_conv_matrix_gpu.py") and "BF16" not in ast.get_source_segment(open(os.path.join(HERE, module)).read(), funcs[fn]) \
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


ATTN_ALL_ROWS = ATTN_ROWS + ATTN_FP8_ROWS + ATTN_FP8_FALLBACK_ROWS
ATTN_LAUNCHERS = {"launch_res256": "attn_res256_kernel<%d, %s, %s>", "launch_dma72": "attn_dma72_kernel<%d, %s, %s>"}     # launcher -> its cvmi_note_kernel format


def attention_source(csrc=CSRC):
    return open(os.path.join(csrc, "attention.hip")).read()


def attention_instances(text):
    """Template instances of the two head-dim-72 launchers cvmi_attention can pick, from its call sites launch_res256<NW[, AV8[, QL]]>( and
    launch_dma72<..>(, each spelled the way the launcher's cvmi_note_kernel format spells it (AV8 and QL default to false)."""
    out = set()
    for fn, args in re.findall(r"\b(launch_res256|launch_dma72)<([^<>]*)>\(", text):
        a = [x.strip() for x in args.split(",")]
        assert 1 <= len(a) <= 3 and a[0].isdigit() and all(x in ("true", "false") for x in a[1:]), (fn, args)
        a += ["false"] * (3 - len(a))
        out.add(ATTN_LAUNCHERS[fn] % (int(a[0]), a[1], a[2]))
    return out


def attention_gaps(text, rows=None):
    """What the attention matrix leaves uncovered among the instances of launch_res256 / launch_dma72, as a list of strings (empty = complete)."""
    rows = ATTN_ALL_ROWS if rows is None else rows
    gaps = [f"attention.hip no longer tags {fmt!r}" for fmt in ATTN_LAUNCHERS.values() if f'cvmi_note_kernel("{fmt}"' not in text]
    inst, tags = attention_instances(text), {r["expect"] for r in rows}
    fams = {re.match(r"\s*(\w+)", f).group(1) for f in re.findall(r'cvmi_note_kernel\(\s*"([^"]*)"', text)}
    gaps += [f"{i} has no row" for i in sorted(inst - tags)]
    for r in rows:
        fam = re.match(r"(\w+)", r["expect"]).group(1)
        if fam in ("attn_res256_kernel", "attn_dma72_kernel"):
            if r["expect"] not in inst:
                gaps.append(f"row {r['id']} expects {r['expect']}, which the dispatcher cannot produce")
        elif r["av_fp8"] and fam not in fams:
            gaps.append(f"row {r['id']} expects {r['expect']}, which attention.hip no longer tags")
    for i in sorted(inst):                                                 # an e4m3 instance is reachable with av_fp8 = 1 only: pinned by such a row
        if _tag_args(i)[1][1] == "true" and not any(r["expect"] == i and r["av_fp8"] for r in rows):
            gaps.append(f"{i} has no av_fp8 = 1 row")
    return gaps


def test_every_res256_and_dma72_instance_is_in_the_dispatch_matrix():
    text = attention_source()
    inst = attention_instances(text)
    assert len(inst) == 8 and {"attn_res256_kernel<8, true, false>", "attn_dma72_kernel<8, true, false>"} <= inst, sorted(inst)      # the parser still finds the call sites
    assert attention_gaps(text) == [], attention_gaps(text)


def test_a_dropped_fp8_row_or_a_new_attention_call_site_is_caught():
    text = attention_source()
    assert attention_gaps(text, ATTN_ROWS + ATTN_FP8_FALLBACK_ROWS) == [
        "attn_dma72_kernel<8, true, false> has no row", "attn_res256_kernel<8, true, false> has no row",
        "attn_dma72_kernel<8, true, false> has no av_fp8 = 1 row", "attn_res256_kernel<8, true, false> has no av_fp8 = 1 row"]
    assert attention_gaps(text, [r for r in ATTN_ALL_ROWS if not r["id"].startswith("dma72_fp8")]) == [
        "attn_dma72_kernel<8, true, false> has no row", "attn_dma72_kernel<8, true, false> has no av_fp8 = 1 row"]
    probe = text + "\n    if (d->av_fp8 && a.qtiles < 8) return launch_res256<4, true>(a, stream);\n"
    assert attention_gaps(probe) == ["attn_res256_kernel<4, true, false> has no row", "attn_res256_kernel<4, true, false> has no av_fp8 = 1 row"]
    probe = text.replace("return launch_dma72<8, true>(a, stream);", "return launch_dma72<8>(a, stream);")
    assert [g for g in attention_gaps(probe) if g.startswith("row dma72_fp8_1024 ")] == ["row dma72_fp8_1024 expects attn_dma72_kernel<8, true, false>, which the dispatcher cannot produce"]
    probe = text.replace('cvmi_note_kernel("attn_dma72_kernel<%d, %s, %s>"', 'cvmi_note_kernel("attn_dma72_kernel<%d>"')
    assert "attention.hip no longer tags 'attn_dma72_kernel<%d, %s, %s>'" in attention_gaps(probe)


def test_matrix_rows_are_well_formed():
    ids = [r["id"] for r in ATTN_ALL_ROWS]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    assert not any(r["av_fp8"] for r in ATTN_ROWS) and all(r["av_fp8"] == 1 for r in ATTN_FP8_ROWS + ATTN_FP8_FALLBACK_ROWS)
    for r in ATTN_ALL_ROWS:
        assert set(r["dtypes"]) <= {"f16", "bf16", "f32"} and r["dtypes"], r["id"]
        assert r["layout"] in ("sep", "qkv", "kv256", "grid"), r["id"]
        assert r["layout"] != "qkv" or r["Nq"] == r["Nk"], r["id"]
        if r["win"]:
            assert r["gh"] % r["win"] == 0 and r["gw"] % r["win"] == 0 and r["Nk"] == r["win"] ** 2, r["id"]
        if r["dtypes"] != ("f32",):
            assert r["dqk"] % 8 == 0 and r["dv"] % 8 == 0 and r["o_pad"] % 8 == 0, r["id"]      # the 16-bit kernels' alignment contract
        if r["av_fp8"]:
            assert set(r["dtypes"]) <= {"f16", "bf16"}, f"{r['id']}: an fp8 row is 16-bit"
            args = _tag_args(r["expect"])[1]
            if len(args) == 3 and args[1] == "true":                                            # what the dispatcher sends to an e4m3 instance
                assert r["dqk"] == 72 and r["dv"] == 72 and (r["Nk"] == 256 or (r["Nk"] >= 512 and r["Nk"] % 64 == 0 and not r["win"])), r["id"]
                assert (r["Nq"] + 31) // 32 >= 8, f"{r['id']}: fewer than 8 query tiles"
                assert r in ATTN_FP8_ROWS, r["id"]
            else:
                assert r in ATTN_FP8_FALLBACK_ROWS, r["id"]
    for r in ATTN_FP8_ROWS:
        assert _tag_args(r["expect"])[1][1:] == ["true", "false"] and not r.get("q_pool"), r["id"]


CONV_SOURCES = ("igemm.hip", "conv_tile.hip")
CONV_FAMILIES = {"conv_tile_kernel", "igemm_kernel", "gemm_glds_kernel", "gemm256_kernel", "gemm256p_kernel", "gemm256x192_kernel", "gemm256x192r_kernel"}


def conv_sources(csrc=CSRC):
    return {name: open(os.path.join(csrc, name)).read() for name in CONV_SOURCES}


def conv_families(sources):
    """Kernel families cvmi_conv2d's dispatcher tags before a launch: the identifier that opens each cvmi_note_kernel("...") format (a launch
    that picks one of two formats with ?: tags the same family either way)."""
    return {re.match(r"\s*(\w+)", s).group(1) for text in sources.values() for s in re.findall(r'cvmi_note_kernel\(\s*(?:\w+\s*\?\s*)?"([^"]*)"', text)}


def conv_instances(sources):
    """Template instances the dispatcher can pick, from its call sites: {("igemm_kernel" | "gemm_glds_kernel" | "conv_tile_kernel", (ints))} --
    launch_cfg<T, TO, BM, BN, WM, WN>, launch_glds<T, TO, BM, BN, WM, WN> and launch_tile<T, KS, S, CC, BN, WM, WN, TH> (the last four: the tile form)."""
    text = "\n".join(sources.values())
    ints = lambda s: tuple(int(v) for v in s.split(","))
    out = {("igemm_kernel", ints(m)) for m in re.findall(r"launch_cfg<T, TO, ([\d, ]+)>\(", text)}
    out |= {("gemm_glds_kernel", ints(m)) for m in re.findall(r"launch_glds<T, TO, ([\d, ]+)>\(", text)}
    out |= {("conv_tile_kernel", ints(m)) for m in re.findall(r"launch_tile<T, KS, S, CC, ([\d, ]+)>\(", text)}
    return out


def _tag_args(tag):
    fam = re.match(r"(\w+)", tag).group(1)
    return fam, [a.strip() for a in tag[len(fam):].strip("<>").split(",")] if "<" in tag else []


def _pair(args):
    """(T, TO) of a tag as "16,16" | "16,float" | "float,float"."""
    return ",".join("float" if a == "float" else "16" for a in args[:2])


def conv_gaps(sources, rows=CONV_ROWS):
    """What the dispatch matrix leaves uncovered, as a list of strings (empty = complete)."""
    tags = {conv_expect(r, dt) for r in rows for dt in r["dtypes"]}
    parsed = [_tag_args(t) for t in tags]
    gaps = []
    fams, covered = conv_families(sources), {f for f, _ in parsed}
    gaps += [f"kernel family {f} has no row" for f in sorted(fams - covered)]
    gaps += [f"rows expect {f}, which the sources no longer tag" for f in sorted(covered - fams)]
    for fam, tup in sorted(conv_instances(sources)):
        want = [str(v) for v in tup]
        if fam == "conv_tile_kernel":                                       # the tile form, in fp16 and (all but the fp16-only 4-row form) in f32
            for T in ("_Float16",) + (("float",) if tup[3] != 4 else ()):
                if not any(f == fam and a[0] == T and a[4:8] == want for f, a in parsed):
                    gaps.append(f"conv_tile_kernel<{T}, .., {', '.join(want)}> has no row")
        else:                                                               # (BM, BN, WM, WN) in each (T, TO) pair
            for pair in ("16,16", "16,float", "float,float"):
                if not any(f == fam and a[2:6] == want and _pair(a) == pair for f, a in parsed):
                    gaps.append(f"{fam}<{pair}, {', '.join(want)}> has no row")
    ig = [a for f, a in parsed if f == "igemm_kernel"]
    gaps += [f"igemm_kernel BKB = {v} has no row" for v in ("64", "128") if not any(a[6] == v for a in ig)]
    gaps += [f"igemm_kernel PLAIN = {v} has no row" for v in ("true", "false") if not any(a[7] == v for a in ig)]
    gaps += [f"igemm_kernel KS = {v} has no row" for v in ("1", "2", "4") if not any(a[8] == v for a in ig)]
    gaps += [f"igemm_kernel KS = {ks} on BN = {bn} has no row" for ks, bn in (("4", "64"), ("2", "64"), ("2", "128")) if not any(a[8] == ks and a[3] == bn for a in ig)]
    ct = [a for f, a in parsed if f == "conv_tile_kernel"]
    for ks_s in (("3", "1"), ("3", "2"), ("2", "1")):
        for cc in ("32", "16", "8"):
            if not any(a[0] == "_Float16" and tuple(a[1:3]) == ks_s and a[3] == cc for a in ct):
                gaps.append(f"conv_tile_kernel<_Float16, {ks_s[0]}, {ks_s[1]}, {cc}, ..> has no row")
    gaps += [f"conv_tile_kernel<float, .., CC = {cc}> has no row" for cc in ("32", "16", "8") if not any(a[0] == "float" and a[3] == cc for a in ct)]
    for t in ("gemm256_kernel<{T}, true>", "gemm256_kernel<{T}, true, true>", "gemm256x192_kernel<{T}>"):
        for T in ("_Float16", "__bf16", "float"):
            if t.replace("{T}", T) not in tags:
                gaps.append(f"{t.replace('{T}', T)} has no row")
    if not any(r["row_stats"] and (r["B"] * r["H"] * r["W"]) % 256 and conv_expect(r, r["dtypes"][0]) == "gemm256x192_kernel<float>" for r in rows if r["B"] != "cu/2"):
        gaps.append("row_stats through gemm256x192_kernel<float>'s LDS epilogue (a ragged last row block) has no row")
    return gaps


def test_every_conv_kernel_family_and_instance_is_in_the_dispatch_matrix():
    src = conv_sources()
    assert conv_families(src) == CONV_FAMILIES, conv_families(src)                 # the parser still finds the seven tagged families
    inst = conv_instances(src)
    assert len([i for i in inst if i[0] == "igemm_kernel"]) == 6 and len([i for i in inst if i[0] == "gemm_glds_kernel"]) == 2 and \
        len([i for i in inst if i[0] == "conv_tile_kernel"]) == 4, sorted(inst)      # ... and the call sites
    assert conv_gaps(src) == [], conv_gaps(src)


def test_a_new_conv_instance_or_a_removed_row_is_caught():
    src = conv_sources()
    probe = dict(src)
    probe["igemm.hip"] += "\n  if (N <= 16) return launch_cfg<T, TO, 32, 32, 1, 1>(a, stream);\n"
    assert conv_gaps(probe) == [f"igemm_kernel<{p}, 32, 32, 1, 1> has no row" for p in ("16,16", "16,float", "float,float")]
    probe = dict(src)
    probe["conv_tile.hip"] = probe["conv_tile.hip"].replace("cvmi_note_kernel(", "note_off(")
    assert "rows expect conv_tile_kernel, which the sources no longer tag" in conv_gaps(probe)
    assert conv_gaps(src, [r for r in CONV_ROWS if r["id"] != "n32_m256"]) == ["igemm_kernel<16,16, 256, 32, 4, 1> has no row", "igemm_kernel<float,float, 256, 32, 4, 1> has no row"]
    assert conv_gaps(src, [r for r in CONV_ROWS if r["id"] != "t31_c32_n64_th8"]) == ["conv_tile_kernel<_Float16, .., 64, 2, 2, 8> has no row"]
    assert conv_gaps(src, [r for r in CONV_ROWS if r["id"] != "g192r"]) == ["kernel family gemm256x192r_kernel has no row"]
    assert "igemm_kernel KS = 4 has no row" in conv_gaps(src, [r for r in CONV_ROWS if not r["id"].startswith("ks4")])
    assert conv_gaps(src, [r for r in CONV_ROWS if r["id"] != "g192_f32_stats_ragged"]) == ["row_stats through gemm256x192_kernel<float>'s LDS epilogue (a ragged last row block) has no row"]


def test_conv_matrix_rows_are_well_formed():
    ids = [r["id"] for r in CONV_ROWS]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    for r in CONV_ROWS:
        rid = r["id"]
        assert r["dtypes"] and set(r["dtypes"]) <= set(TNAME), rid
        assert not isinstance(r["expect"], dict) or set(r["expect"]) == set(r["dtypes"]), rid
        cins = r["Cin"] if isinstance(r["Cin"], tuple) else (r["Cin"],)
        for dt in r["dtypes"]:
            tag = conv_expect(r, dt)
            assert "{" not in tag and _tag_args(tag)[0] in CONV_FAMILIES, (rid, tag)
            assert dt != "bf16" or not tag.startswith("conv_tile_kernel"), f"{rid}: the bf16 build has no conv_tile path"
            assert r["scalar_gather"] or all(c % (4 if dt == "f32" else 8) == 0 for c in cins), f"{rid}: channels not in 16-byte vectors"
            ovec = 4 if (dt == "f32" or r["out_f32"]) else 8
            assert r["y_pad"] % ovec == 0, f"{rid}: y_pad breaks the output's 16-byte alignment"
            assert not r["shuffle_cout"] or r["shuffle_cout"] % ovec == 0, rid
        assert r["act"] in ("none", "relu", "silu", "gelu") and r["res"] in ("none", "full", "bcast", "rep"), rid
        assert (r["up"] is None) if len(cins) == 1 else (r["up"] in (None, 0, 1)), rid
        assert r["up"] is None or (r["H"] % 2 == 0 and r["W"] % 2 == 0), rid
        if r["shuffle_cout"]:
            assert r["k"] == 1 and r["stride"] == 1 and r["pad"] == 0 and r["Cout"] == 4 * r["shuffle_cout"] and r["res"] != "bcast", rid
        assert (r["res"] == "rep") == (r["res_rep"] > 1), rid
        if r["res"] == "rep":
            assert isinstance(r["B"], int) and r["B"] % r["res_rep"] == 0, rid
        assert r["B"] == "cu/2" or (isinstance(r["B"], int) and r["B"] > 0), rid
        assert not r["out_f32"] or "f32" not in r["dtypes"] or isinstance(r["expect"], dict), rid
        if r["row_stats"]:                                                  # what engine.op_conv / launch_typed admit statistics with
            M = r["B"] * r["H"] * r["W"]
            assert r["out_f32"] and r["res"] == "full" and r["k"] == 1 and r["Cout"] % 192 == 0 and not r["y_pad"] and not r["shuffle_cout"], rid
            from circuitvision_amd.engine import row_stats_supported
            assert row_stats_supported(M, r["Cout"], r["Cin"]), rid


FUSED_SOURCES = ("c3k2_fused.hip", "stem_fused.hip", "dwpw_fused.hip")


def fused_sources(csrc=CSRC):
    return {name: open(os.path.join(csrc, name)).read() for name in FUSED_SOURCES}


def fused_instances(sources):
    """Tags of the instances the three fused entry points can launch, from their call sites: launch_c3k2<C, HR, C2, C1>(, launch_dwpw<CC, NCHUNK,
    N1P, N2P>( and the hipLaunchKernelGGL(stem2_kernel, ..) launch -- spelled as the launchers' cvmi_note_kernel formats spell them."""
    ints = lambda s: tuple(int(v) for v in s.split(","))
    out = ["c3k2_kernel<%d, %d, %d, %d>" % ints(m) for m in re.findall(r"launch_c3k2<([\d, ]+)>\(", sources["c3k2_fused.hip"])]
    out += ["dwpw_kernel<%d, %d, %d, %d>" % ints(m) for m in re.findall(r"launch_dwpw<([\d, ]+)>\(", sources["dwpw_fused.hip"])]
    out += ["stem2_kernel"] * len(re.findall(r"hipLaunchKernelGGL\(\s*stem2_kernel\s*,", sources["stem_fused.hip"]))
    return out


def fused_gaps(sources, rows=FUSED_ROWS):
    """What the fused matrix leaves uncovered, as a list of strings (empty = complete)."""
    gaps = []
    for name, fmt in (("c3k2_fused.hip", "c3k2_kernel<%d, %d, %d, %d>"), ("dwpw_fused.hip", "dwpw_kernel<%d, %d, %d, %d>"), ("stem_fused.hip", "stem2_kernel")):
        if 'cvmi_note_kernel("%s"' % fmt not in sources[name]:
            gaps.append(f"{name} no longer tags its launch as {fmt}")
    inst, tags = set(fused_instances(sources)), {r["expect"] for r in rows}
    gaps += [f"{t} has no row" for t in sorted(inst - tags)]
    gaps += [f"rows expect {t}, which the sources no longer launch" for t in sorted(tags - inst)]
    for t in sorted(t for t in inst & tags if t.startswith("c3k2_kernel")):             # what every c3k2 instance needs beside a row
        mine = [r for r in rows if r["expect"] == t]
        if not any(r["B"] == "persist" for r in mine):
            gaps.append(f"{t} has no persistent row")
        if not any(r["shortcut"] == 0 for r in mine):
            gaps.append(f"{t} has no shortcut = 0 row")
    return gaps


def test_every_fused_kernel_instance_is_in_the_fused_matrix():
    src = fused_sources()
    inst = fused_instances(src)
    assert len(inst) == len(set(inst)), inst
    assert [sum(t.startswith(f) for t in inst) for f in ("c3k2_kernel", "dwpw_kernel", "stem2_kernel")] == [5, 8, 1], inst      # the parser still finds the call sites
    assert {t for t in inst if t.startswith("c3k2")} == {c3k2_tag(i) for i in C3K2_INSTANCES}
    assert fused_gaps(src) == [], fused_gaps(src)


def test_a_new_fused_instance_or_a_removed_row_is_caught():
    src = fused_sources()
    probe = dict(src)
    probe["c3k2_fused.hip"] += "\n  if (d->c == 64) return launch_c3k2<64, 32, 128, 0>(a, d->B, s);\n"
    assert fused_gaps(probe) == ["c3k2_kernel<64, 32, 128, 0> has no row"]
    probe = dict(src)
    probe["dwpw_fused.hip"] += "\n  return launch_dwpw<80, 2, 96, 0>(a, d->B, s);\n"
    assert fused_gaps(probe) == ["dwpw_kernel<80, 2, 96, 0> has no row"]
    probe = dict(src)
    probe["stem_fused.hip"] = probe["stem_fused.hip"].replace('cvmi_note_kernel("stem2_kernel")', "")
    assert fused_gaps(probe) == ["stem_fused.hip no longer tags its launch as stem2_kernel"]
    assert fused_gaps(src, [r for r in FUSED_ROWS if r["id"] != "dwpw_c64_n80"]) == ["dwpw_kernel<64, 1, 96, 0> has no row"]
    assert fused_gaps(src, [r for r in FUSED_ROWS if r["kernel"] != "stem2"]) == ["stem2_kernel has no row"]
    assert fused_gaps(src, [r for r in FUSED_ROWS if r["id"] != "c3k2_32_16_128_0_persist"]) == ["c3k2_kernel<32, 16, 128, 0> has no persistent row"]
    assert fused_gaps(src, [r for r in FUSED_ROWS if r["id"] != "c3k2_16_8_64_0_9x17_noshort"]) == ["c3k2_kernel<16, 8, 64, 0> has no shortcut = 0 row"]
    assert fused_gaps(src, [r for r in FUSED_ROWS if r.get("inst") != (32, 16, 64, 0)]) == ["c3k2_kernel<32, 16, 64, 0> has no row"]


def test_fused_matrix_rows_are_well_formed():
    ids = [r["id"] for r in FUSED_ROWS]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    for r in FUSED_ROWS:
        rid = r["id"]
        assert r["kernel"] in ("c3k2", "stem2", "dwpw") and r["expect"].startswith(r["kernel"] + "_kernel"), rid
        assert r["x_off"] % 8 == 0 and r["x_extra"] % 8 == 0 and r["y_guard"] % 8 == 0, f"{rid}: offsets and guards keep the 16-byte alignment"
        assert 0 <= r["x_off"] <= r["x_extra"], rid
        assert r["H"] > 0 and r["W"] > 0, rid
        if r["B"] == "persist":
            assert r["kernel"] == "c3k2" and r["k"] == c3k2_max_wgs_per_cu(r["inst"]) == (8 if r["inst"][0] == 16 else 4), f"{rid}: k must match the thread count"
            assert -(-r["H"] // 8) * -(-r["W"] // 16) > 1, f"{rid}: more than one tile per image, so consecutive tiles of a workgroup change image AND origin"
        else:
            assert isinstance(r["B"], int) and r["B"] >= 2, f"{rid}: B >= 2 with different images"
        if r["kernel"] == "c3k2":
            c, h, c2, c1 = r["inst"]
            assert r["inst"] in C3K2_INSTANCES and r["expect"] == c3k2_tag(r["inst"]) and r["shortcut"] in (0, 1), rid
            assert (c1 > 0) == (c1 in (32, 64)), f"{rid}: fuse_cv1 rows carry c1"
        if r["kernel"] == "dwpw":
            assert r["N1"] % 8 == 0 and 0 <= r["N2"] <= 64, rid
    for mut, rids in FUSED_MUTANT_ROWS.items():
        assert rids and set(rids) <= set(ids), mut


# ---- the helper kernels: sam_ops.hip launch_ln / cvmi_upsample_refine, vision_ops.hip cvmi_sppf_pool ---------------------------------------------------
HELPER_SOURCES = ("sam_ops.hip", "vision_ops.hip")
LN_PAIRS = [(4, 1), (4, 3), (4, 5), (4, 9), (8, 1), (8, 3), (8, 5), (8, 9), (16, 1), (16, 3), (16, 5), (16, 9), (32, 1), (32, 3), (32, 5), (32, 8), (32, 9),
            (64, 1), (64, 2), (64, 3), (64, 5), (64, 8), (64, 9)]
HELPER_TAGS = {"sam_ops.hip": ("layernorm_kernel<%s, %s, %d, %d>", "upsample_refine_fast_kernel", "upsample_refine_kernel<4>"),
               "vision_ops.hip": ("sppf_pool_lds_kernel<%s>", "sppf_pool_kernel<%s>")}


def helper_sources(csrc=CSRC):
    return {name: open(os.path.join(csrc, name)).read() for name in HELPER_SOURCES}


def ln_switch(sources):
    """(instances of CVMI_LN_SW: the NCH of every case and of the default, the candidate list of launch_ln's selection loop) from sam_ops.hip."""
    text = sources["sam_ops.hip"]
    body = re.search(r"#define CVMI_LN_SW\(W\)(.*?)\n  \}\n", text, re.S).group(1)
    inst = [int(m) for m in re.findall(r"(?:case \d+|default):\s*CVMI_LN\((\d+), W\)", body)]
    assert all(c == n for c, n in re.findall(r"case (\d+):\s*CVMI_LN\((\d+), W\)", body)), "a case launches another instance than it names"
    ncand = [int(v) for v in re.search(r"const int ncand\[\d+\] = \{([\d, ]+)\}", text).group(1).split(",")]
    return inst, ncand


def helper_gaps(sources, ln_rows=LN_ROWS, rows=HELPER_ROWS):
    """What the helper matrix leaves uncovered, as a list of strings (empty = complete)."""
    gaps = []
    for name, fmts in HELPER_TAGS.items():
        gaps += [f"{name} no longer tags its launch as {fmt}" for fmt in fmts if 'cvmi_note_kernel("%s"' % fmt not in sources[name]]
    inst, ncand = ln_switch(sources)
    have = {(r["form"], r["G"], r["NCH"]) for r in ln_rows}
    gaps += [f"layernorm_kernel<.., {n}, ..> has no row" for n in sorted(set(inst) - {h[2] for h in have})]
    gaps += [f"launch_ln tries NCH = {n}, which CVMI_LN_SW does not build" for n in sorted(set(ncand) - set(inst))]
    for form in LN_FORMS:
        gaps += [f"layernorm {form} (G, NCH) = ({G}, {n}) has no row" for G, n in sorted(ln_reachable(ncand)) if (form, G, n) not in have]
    tags = {r["expect"] for r in rows}
    for fam in ("sppf_pool_lds_kernel", "sppf_pool_kernel"):
        gaps += [f"{fam}<{TNAME[dt]}> has no row" for dt in ("f16", "f32") if f"{fam}<{TNAME[dt]}>" not in tags]
    gaps += [f"{t} has no row" for t in ("upsample_refine_fast_kernel", "upsample_refine_kernel<4>") if t not in tags]
    sppf = [r for r in rows if r["op"] == "sppf_pool"]
    for dt, px in SPPF_LDS_PIXELS.items():
        if not any(r["dtypes"] == (dt,) and r["H"] * r["W"] == px for r in sppf):
            gaps.append(f"sppf_pool {dt}: no row at the LDS limit of {px} pixels")
        if not any(r["dtypes"] == (dt,) and px < r["H"] * r["W"] <= px + r["W"] for r in sppf):
            gaps.append(f"sppf_pool {dt}: no row one image row past the LDS limit of {px} pixels")
    return gaps


def test_ln_pick_mirrors_launch_ln():
    inst, ncand = ln_switch(helper_sources())
    assert tuple(ncand) == LN_NCAND and sorted(inst) == sorted(LN_NCAND), (inst, ncand)
    assert sorted(ln_reachable()) == LN_PAIRS
    # the widths the older per-op tests run, as the issue that introduced this matrix lists them
    assert [ln_pick(c, 4)[:2] for c in (16, 64, 144, 256, 1152)] == [(4, 1), (16, 1), (4, 9), (64, 1), (32, 9)]
    assert [ln_pick(c, 8)[:2] for c in (16, 64, 144, 256, 1152)] == [(4, 1), (8, 1), (4, 5), (32, 1), (16, 9)]
    assert all(ln_pick(c, s)[1] == 3 for c in (96, 192, 384, 768) for s in (4, 8))        # Hiera-T / S / B+
    for r in LN_ROWS:                                                      # every row carries what ln_pick says, and G is the smallest that fits NCH
        slot = LN_FORMS[r["form"]][2]
        assert (r["G"], r["NCH"], r["waste"]) == ln_pick(r["C"], slot), r["id"]
        assert r["G"] == min(G for G in (4, 8, 16, 32, 64) if G * r["NCH"] * slot >= r["C"]), r["id"]
        assert all(ln_tag(r["form"], r["NCH"], dt).startswith("layernorm_kernel<") for dt in r["dtypes"])
    assert all(r["expect"] == ln_tag("f32_f32", r["NCH"], "f32") for r in LN_DUAL_ROWS)


def test_every_helper_kernel_and_layernorm_instance_is_in_the_helper_matrix():
    src = helper_sources()
    assert helper_gaps(src) == [], helper_gaps(src)
    for form in LN_FORMS:                                                  # ... each reachable pair at the smallest width that selects it
        slot = LN_FORMS[form][2]
        for (G, n), chunks in ln_reachable().items():
            assert any(r["form"] == form and r["C"] == chunks[0] * slot and (r["G"], r["NCH"]) == (G, n) for r in LN_ROWS), (form, G, n)
        for tag in ("rows1", "wg_minus1", "wg_plus1", "waste", "inside", "padgrid", "gelu"):
            assert {r["NCH"] for r in LN_ROWS if r["form"] == form and r["id"].endswith("_" + tag)} == {3, 2}, (form, tag)
    assert all(r["dtypes"] == (("f32",) if r["form"] == "f32_f32" else ("f16", "bf16")) for r in LN_ROWS)


def test_a_new_layernorm_case_or_a_removed_helper_row_is_caught():
    src = helper_sources()
    probe = dict(src)
    probe["sam_ops.hip"] = probe["sam_ops.hip"].replace("    case 5: CVMI_LN(5, W); break;", "    case 4: CVMI_LN(4, W); break;  \\\n    case 5: CVMI_LN(5, W); break;")
    assert probe != src and helper_gaps(probe) == ["layernorm_kernel<.., 4, ..> has no row"]
    probe["sam_ops.hip"] = probe["sam_ops.hip"].replace("ncand[6] = {1, 2, 3, 5, 8, 9}", "ncand[7] = {1, 2, 3, 4, 5, 8, 9}")
    assert "layernorm f32_f32 (G, NCH) = (64, 4) has no row" in helper_gaps(probe) and "layernorm_kernel<.., 4, ..> has no row" in helper_gaps(probe)
    for name, fmts in HELPER_TAGS.items():
        for fmt in fmts:
            probe = dict(src)
            probe[name] = probe[name].replace('cvmi_note_kernel("%s"' % fmt, 'note_off("%s"' % fmt)
            assert helper_gaps(probe) == [f"{name} no longer tags its launch as {fmt}"]
    for form in LN_FORMS:                                                  # deleting any one (G, NCH) row names it
        for G, n in LN_PAIRS:
            rid = next(r["id"] for r in LN_ROWS if r["form"] == form and (r["G"], r["NCH"]) == (G, n) and r["id"].endswith("_min"))
            left = [r for r in LN_ROWS if r["id"] != rid and not ((r["G"], r["NCH"]) == (G, n) and r["form"] == form)]
            assert f"layernorm {form} (G, NCH) = ({G}, {n}) has no row" in helper_gaps(src, left)
    drop = lambda rid: helper_gaps(src, rows=[r for r in HELPER_ROWS if r["id"] != rid])
    assert drop("sppf_past_lds_limit_f16") == ["sppf_pool f16: no row one image row past the LDS limit of 1024 pixels"]
    assert drop("sppf_past_lds_limit_f32") == ["sppf_pool_kernel<float> has no row", "sppf_pool f32: no row one image row past the LDS limit of 2048 pixels"]
    assert drop("sppf_lds_limit_f32") == ["sppf_pool f32: no row at the LDS limit of 2048 pixels"]
    assert helper_gaps(src, rows=[r for r in HELPER_ROWS if r["expect"] != "upsample_refine_kernel<4>"]) == ["upsample_refine_kernel<4> has no row"]
    assert helper_gaps(src, rows=[r for r in HELPER_ROWS if r["expect"] != "upsample_refine_fast_kernel"]) == ["upsample_refine_fast_kernel has no row"]


def test_the_native_library_reads_no_tuning_switch():
    """Dispatch depends on shapes alone: a getenv in the HIP sources would bring back a run-time A/B switch (and the kernel variants only it
    reaches, shipped untested).  A/B runs load a second build through CVMI_LIB_PATH instead."""
    sources = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))}
    assert "getenv(\"CVMI_MLP_PIPE\")" in sources["hiera_mlp.hip"]          # the scan sees the one allowed read
    assert stray_getenv(sources) == [], stray_getenv(sources)
    probe = {"x.hip": 'int a = atoi(getenv("CVMI_X"));\n#ifdef CVMI_MLP_DIAGS\n#if 1\n#endif\ngetenv("D");\n#endif\ngetenv ("Y");\n',
             "hiera_mlp.hip": 'getenv("CVMI_MLP_PIPE"); getenv("CVMI_MLP_VAR");\n'}
    assert stray_getenv(probe) == [("hiera_mlp.hip", 1), ("x.hip", 1), ("x.hip", 5), ("x.hip", 7)]


# ---- the token-stationary path: tok_linear.hip, tok_linear16.hip, hiera_mlp.hip, tok_stream.hpp ------------------------------------------------
TOK_SOURCES = ("tok_linear.hip", "tok_linear16.hip", "hiera_mlp.hip", "tok_stream.hpp")
TOK_TAGS = {"tok_linear.hip": "tok_linear_kernel<%d, %d, %s, %s, %s, %s>", "tok_linear16.hip": "tok_linear16_kernel<%d, %d, %s, %s, %s>",
            "hiera_mlp.hip": "hiera_mlp_kernel<%d, %d>"}
TOK_TAG_ARGS = {"tok_linear.hip": "K, LN, CVMI_BOOLNAME(RES), CVMI_BOOLNAME(GELU), CVMI_BOOLNAME(TSTORE), CVMI_BOOLNAME(POOL)",
                "tok_linear16.hip": "K, LN, CVMI_BOOLNAME(RES), CVMI_BOOLNAME(GELU), CVMI_BOOLNAME(POOL)", "hiera_mlp.hip": "C, VAR"}
# launch_tl (tok_linear.hip): the staged store for 16-bit outputs whose N and stride are multiples of 8, the direct store otherwise
TSTORE_RULE = """  if constexpr (!RES) {
    if (d.N % 8 == 0 && d.out_ld % 8 == 0) return launch_tl1<K, LN, RES, GELU, true>(d, s, ex);
  }
  return launch_tl1<K, LN, RES, GELU, false>(d, s, ex);"""
TL16_SPLITS_BODY = """  const long long wg = rows / 256;
  const int nch = (N + 31) / 32;
  if (wg >= 256 || wg % 8 != 0 || (stats_out && N % 32 != 0)) return 1;
  int best = 1;
  for (int ns = 2; ns <= 8 && ns <= nch; ++ns)
    if (nch % ns == 0 && wg * ns <= 256) best = ns;"""
_DECL = "decltype(LN)::value, decltype(RES)::value, decltype(GELU)::value"
_B = {"true": True, "false": False}


def tok_sources(csrc=CSRC):
    return {name: open(os.path.join(csrc, name)).read() for name in TOK_SOURCES}


def tok_dispatch_forms(sources):
    """The (LN, RES, GELU) triples tok_dispatch (tok_stream.hpp) can hand to its launcher, from the launch(..) calls of its return statements."""
    body = re.search(r"int tok_dispatch\(bool ln, bool res, bool gelu, Launch&& launch\) \{(.*?)\n\}", sources["tok_stream.hpp"], re.S).group(1)
    return [(int(a[2]), b == "yes", c == "yes") for a, b, c in re.findall(r"launch\((ln[01]), (yes|no), (yes|no)\)", body)]


def tok_instances(sources):
    """Tags of every instance the three dispatchers can launch, from their call sites, spelled as their cvmi_note_kernel formats spell them."""
    tl, t16, mlp = sources["tok_linear.hip"], sources["tok_linear16.hip"], sources["hiera_mlp.hip"]
    forms = tok_dispatch_forms(sources)
    nb = lambda v: "true" if v else "false"
    out = []
    for K in re.findall(r"dispatch_tl<(\d+)>\(", tl):                       # launch_tl<K, ..> through tok_dispatch, and the ln == 2 branch
        mine = list(forms) if "launch_tl<K, %s>(" % _DECL in tl else []
        mine += [(int(l), _B[r], _B[g]) for l, r, g in re.findall(r"launch_tl<K, (\d), (true|false), (true|false)>\(", tl)]
        for LN, RES, GELU in mine:
            for ts in ((False,) if RES else (True, False)) if TSTORE_RULE in tl else ():
                out.append("tok_linear_kernel<%s, %d, %s, %s, %s, false>" % (K, LN, nb(RES), nb(GELU), nb(ts)))
    for m in re.findall(r"launch_tl1<(\d+), (\d), (true|false), (true|false), (true|false)(?:, (true|false))?>\(", tl):
        out.append("tok_linear_kernel<%s, %s, %s, %s, %s, %s>" % (m[:5] + (m[5] or "false",)))
    for K, pool in re.findall(r"launch16<(\d+), %s, (true|false)>\(" % re.escape(_DECL), t16):
        out += ["tok_linear16_kernel<%s, %d, %s, %s, %s>" % (K, LN, nb(RES), nb(GELU), pool) for LN, RES, GELU in forms]
    out += ["tok_linear16_kernel<%s, %s, %s, %s, %s>" % m for m in re.findall(r"launch16<(\d+), (\d), (true|false), (true|false), (true|false)>\(", t16)]
    out += ["hiera_mlp_kernel<%s, %s>" % m for m in re.findall(r"launch_mlp<(\d+), (\d)>\(", mlp)]
    return out


def tok_gaps(sources, rows=TOK_ROWS, mlp_rows=MLP_ROWS):
    """What the token-path matrix leaves uncovered, as a list of strings (empty = complete)."""
    gaps = []
    for name, fmt in TOK_TAGS.items():
        if 'cvmi_note_kernel("%s", %s)' % (fmt, TOK_TAG_ARGS[name]) not in sources[name]:
            gaps.append(f"{name} no longer tags its launch as {fmt}")
    inst, tags = set(tok_instances(sources)), {r["expect"] for r in rows} | {r["expect"] for r in mlp_rows}
    gaps += [f"{t} has no row" for t in sorted(inst - tags)]
    gaps += [f"rows expect {t}, which the sources no longer launch" for t in sorted(tags - inst)]
    for K in TOK_KS:
        fmt = TOK_FORMAT[K]
        for fam in TOK_NCH_FAMILIES:
            if fam == "direct" and fmt == 16:
                continue
            have = {(r["N"] + 31) // 32 for r in rows if r["K"] == K and r["rows"] == 256 and tok_nch_family(r) == fam}
            gaps += [f"K = {K} {fam}: no one-workgroup row with {n} chunks (ring of {TOK_SLOTS[fmt]} slots)" for n in TOK_NCH[fmt] if n not in have]
        if not any(r["K"] == K and r["pool"] and (r["grid"][2] // 2) & (r["grid"][2] // 2 - 1) for r in rows):
            gaps.append(f"K = {K}: no POOL row whose half width is no power of two")
        gaps += [f"K = {K}: no row that takes {P} per-slice statistics" for P in TOK_PARTS if not any(r["K"] == K and r["stats_in"] == P for r in rows)]
    for ns in sorted({ns for _, _, ns in TOK_SPLIT_TABLE if ns > 1}):
        if not any(r["ns"] == ns for r in rows):
            gaps.append(f"K = 576: no row whose row blocks are shared by {ns} workgroups")
    return gaps


def test_tok_pick_mirrors_the_dispatchers():
    src = tok_sources()
    tl, t16, mlp = src["tok_linear.hip"], src["tok_linear16.hip"], src["hiera_mlp.hip"]
    forms = tok_dispatch_forms(src)
    assert len(forms) == 6 and len(set(forms)) == 5 + 1, forms             # the parser still finds tok_dispatch's launches: three returns, six calls
    assert set(forms) == {tok_dispatch(ln, res, gelu) for ln in (0, 1) for res, gelu in ((False, False), (False, True), (True, False))}
    body = re.search(r"int tok_dispatch\(.*?\n\}", src["tok_stream.hpp"], re.S).group(0)
    assert "if (res) return ln ? launch(ln1, yes, no) : launch(ln0, yes, no);" in body and "if (ln) return gelu ? launch(ln1, no, yes) : launch(ln1, no, no);" in body \
        and "return gelu ? launch(ln0, no, yes) : launch(ln0, no, no);" in body
    assert TSTORE_RULE in tl and tl.count("launch_tl1<K, LN, RES, GELU,") == 2          # launch_tl's rule, as tok_pick states it
    assert "if (ln == 2) return launch_tl<K, 2, false, false>(" in tl and "return tok_dispatch(ln != 0, res, act == CVMI_ACT_GELU," in tl
    assert "if (K == 144) return dispatch_tl<144>(" in tl and "return dispatch_tl<288>(" in tl and "if (tl_format(K) == 16)" in tl
    assert "static int tl_format(int K) { return K == 576 ? 16 : 32; }" in tl
    assert "if (K == 144) return launch_tl1<144, 1, false, false, false, true>(" in tl and "return launch_tl1<288, 1, false, false, false, true>(" in tl
    assert "if (pool_w > 0) return launch16<576, 1, false, false, true>(" in t16 and "return tok_dispatch(ln != 0, res, gelu," in t16
    assert 'CVMI_CHECK(res || (N % 8 == 0 && out_ld % 8 == 0), "tok_linear (16x16x32 format)' in t16
    assert TL16_SPLITS_BODY in t16 and "const int ns = tl16_splits(rows, N, RES && ex.stats_out != nullptr);" in t16
    assert "int CVMI_ENTRY(cvmi_tok_linear16_splits)(long long rows, int N) { return tl16_splits(rows, N, true); }" in t16
    assert "if (C == 144) return launch_mlp<144, 1>(" in mlp and "if (pipe && !(atoi(pipe) & 2)) return launch_mlp<288, 0>(" in mlp and "return launch_mlp<288, 2>(" in mlp
    assert "static constexpr int SLOTS = 4;" in tl and "static constexpr int SLOTS = 3;" in t16 and "tok_pingpong<RES, SLOTS - 1>(" in tl and "tok_pingpong<RES, SLOTS - 1>(" in t16
    assert TOK_SLOTS == {32: 4, 16: 3}
    inst = tok_instances(src)
    assert len(inst) == len(set(inst)), inst
    assert [sum(t.startswith(f) for t in inst) for f in ("tok_linear_kernel<", "tok_linear16_kernel<", "hiera_mlp_kernel<")] == [26, 7, 3], inst   # the parser still finds the call sites
    assert sorted(t for t in inst if t.startswith("tok_linear")) == TOK_INSTANCES and sorted(t for t in inst if t.startswith("hiera")) == MLP_INSTANCES
    assert [mlp_pick(144), mlp_pick(288), mlp_pick(288, "0"), mlp_pick(288, "2"), mlp_pick(288, "1")] == \
        ["hiera_mlp_kernel<144, 1>", "hiera_mlp_kernel<288, 2>", "hiera_mlp_kernel<288, 0>", "hiera_mlp_kernel<288, 2>", "hiera_mlp_kernel<288, 0>"]
    assert [tl16_splits(rows, N, False) for rows, N, _ in TOK_SPLIT_TABLE] == [ns for _, _, ns in TOK_SPLIT_TABLE]
    assert tl16_splits(2048, 40, True) == 1 and tl16_splits(2048, 576, True) == 6 and tl16_splits(65536, 576, True) == 1 and tl16_splits(32768, 576, True) == 2


def test_every_token_path_instance_is_in_the_matrix():
    assert tok_gaps(tok_sources()) == [], tok_gaps(tok_sources())


def test_a_new_token_path_instance_or_a_removed_row_is_caught():
    src = tok_sources()
    probe = dict(src)
    probe["tok_linear.hip"] += "\n  if (res && gelu) return launch_tl1<144, 1, true, true, false>(d, s, ex);\n"
    assert tok_gaps(probe) == ["tok_linear_kernel<144, 1, true, true, false, false> has no row"]
    probe = dict(src)
    probe["hiera_mlp.hip"] += "\n  return launch_mlp<288, 1>(*d, s);\n"
    assert tok_gaps(probe) == ["hiera_mlp_kernel<288, 1> has no row"]
    for name, fmt in TOK_TAGS.items():
        probe = dict(src)
        probe[name] = probe[name].replace('cvmi_note_kernel("%s"' % fmt, 'note_off("%s"' % fmt)
        assert probe != src and tok_gaps(probe) == [f"{name} no longer tags its launch as {fmt}"]
    probe = dict(src)
    probe["tok_linear.hip"] = probe["tok_linear.hip"].replace("d.N % 8 == 0 && d.out_ld % 8 == 0) return launch_tl1", "d.N % 16 == 0 && d.out_ld % 8 == 0) return launch_tl1")
    assert len(tok_gaps(probe)) == 24 and all("which the sources no longer launch" in g for g in tok_gaps(probe))       # the rule's text is part of the mirror
    drop = lambda *rids: tok_gaps(src, [r for r in TOK_ROWS if r["id"] not in rids], [r for r in MLP_ROWS if r["id"] not in rids])
    assert drop("k144_ln1_gelu_n40_ld48_inst") == []                      # (the chunk-count rows launch this instance too)
    assert drop("k288_ln2_n36_ld40_inst", "k288_ln2_n32_ld36_inst") == ["tok_linear_kernel<288, 2, false, false, false, false> has no row"]
    assert drop("k288_ln0_n136_ld140_nch", "k288_ln0_n160_ld164_nch") == ["K = 288 direct: no one-workgroup row with 5 chunks (ring of 4 slots)"]
    assert drop("k576_ln1_res_n128_ld132_nch", "k576_ln1_res_n104_ld108_nch") == ["K = 576 res_ln1: no one-workgroup row with 4 chunks (ring of 3 slots)"]
    assert drop("k576_ln1_gelu_n224_ld232_split7") == ["K = 576: no row whose row blocks are shared by 7 workgroups"]
    assert drop(*[r["id"] for r in TOK_ROWS if r["K"] == 144 and r["grid"] == (2, 64, 6)]) == ["K = 144: no POOL row whose half width is no power of two"]
    assert drop("k288_ln1_n72_ld80_parts3") == ["K = 288: no row that takes 3 per-slice statistics"]
    assert drop(*[r["id"] for r in MLP_ROWS if r["expect"] == "hiera_mlp_kernel<288, 0>"]) == ["hiera_mlp_kernel<288, 0> has no row"]


def test_token_path_rows_are_well_formed():
    ids = [r["id"] for r in TOK_ROWS] + [r["id"] for r in MLP_ROWS]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    for r in TOK_ROWS:
        rid, K, N = r["id"], r["K"], r["N"]
        assert r["dtypes"] == ("f16", "bf16") and r["fam"] in ("inst", "nch", "layout", "stats", "split", "pool"), rid
        assert r["rows"] % 256 == 0 and (r["rows"] <= 2304 or rid == "k576_ln0_n256_ld264_split4_rows16384"), rid   # (2304: nine row blocks)
        assert r["in_ld"] >= K and r["in_ld"] % (4 if r["ln"] else 8) == 0 and r["out_ld"] >= N and r["out_ld"] % 4 == 0 and N % 4 == 0, f"{rid}: the alignment contract"
        assert TOK_FORMAT[K] == 32 or r["res"] or r["pool"] or (N % 8 == 0 and r["out_ld"] % 8 == 0), f"{rid}: K = 576 16-bit outputs in 16-byte pieces"
        assert r["expect"] == tok_pick(K, r["ln"], r["res"], r["gelu"], N, r["out_ld"], r["pool"]) and r["expect"] in TOK_INSTANCES, rid
        assert r["ns"] == (tl16_splits(r["rows"], N, r["res"] and r["stats_out"]) if TOK_FORMAT[K] == 16 else None), rid
        assert r["stats_in"] in (None, "pair") + TOK_PARTS and (r["stats_in"] is None or r["ln"] == 1) and (not r["stats_out"] or r["res"]), rid
        assert not isinstance(r["stats_in"], int) or K % r["stats_in"] == 0, rid
        assert r["row_off"] % 256 == 0 and (not r["chain"] or (r["stats_out"] and r["ns"] > 1 and K == N == r["out_ld"])), rid
        if r["pool"]:
            B, H, W = r["grid"]
            assert H % 2 == 0 and W % 2 == 0 and B * H * W == r["rows"] and r["ln"] == 1 and not (r["res"] or r["gelu"] or r["stats_out"] or r["row_off"]), rid
        else:
            assert r["grid"] is None, rid
    for rows, N, ns in TOK_SPLIT_TABLE:                                      # every split the table claims has its row, and the chain row writes 6 parts
        assert any(r["K"] == 576 and (r["rows"], r["N"], r["ns"]) == (rows, N, ns) for r in TOK_ROWS), (rows, N, ns)
    assert [r["ns"] for r in TOK_ROWS if r["chain"]] == [6] and any(r["stats_out"] and r["ns"] == 1 and r["rows"] == 2048 and r["N"] == 40 for r in TOK_ROWS)
    assert any(r["pool"] and r["ns"] == 3 for r in TOK_ROWS)
    for K in TOK_KS:                                                        # layout: three workgroups, padded input behind an offset view, guards; statistics out at N = 136 and N = K
        lay = [r for r in TOK_ROWS if r["K"] == K and r["fam"] == "layout"]
        assert lay and all(r["rows"] == 768 and r["in_ld"] == K + (4 if r["ln"] else 8) and r["row_off"] > 0 and r["out_ld"] > r["N"] for r in lay), K
        assert {(r["ln"], r["res"]) for r in lay} >= {(0, False), (1, False), (0, True), (1, True)} and any(r["stats_out"] for r in lay), K
        assert {(r["N"], r["out_ld"]) for r in TOK_ROWS if r["K"] == K and r["stats_out"] and r["fam"] == "stats"} == {(136, 144), (K, K)}, K
        assert any(r["K"] == K and r["stats_in"] == "pair" and not r["pool"] for r in TOK_ROWS) and any(r["K"] == K and r["stats_in"] == "pair" and r["pool"] for r in TOK_ROWS), K
        assert {r["grid"] for r in TOK_ROWS if r["K"] == K and r["fam"] == "pool"} == {(1, 16, 16), (2, 64, 6), (3, 8, 32), (1, 2, 128)}, K
        if TOK_FORMAT[K] == 32:
            assert {r["ln"] for r in TOK_ROWS if r["K"] == K and r["N"] == 144 and r["res"] and r["fam"] == "nch"} == {0, 1}, f"K = {K}: the residual form's half chunk"
    for r in MLP_ROWS:
        assert r["expect"] == mlp_pick(r["C"], r["pipe"]) and r["expect"] in MLP_INSTANCES and r["x_ld"] >= r["C"] and r["x_ld"] % 4 == 0 and r["dtypes"] == ("f16", "bf16"), r["id"]
    for tag in MLP_INSTANCES:
        mine = [r for r in MLP_ROWS if r["expect"] == tag]
        assert {r["rows"] for r in mine if r["stats_out"] and r["x_ld"] > r["C"]} == {1, 5, 31, 32, 33, 127, 128, 129, 391}, tag
        assert any(not r["stats_out"] for r in mine) and any(r["x_ld"] == r["C"] for r in mine), tag
    for mut, rids in list(TOK_MUTANT_ROWS.items()) + list(TOK_UNSEEN_MUTANTS.items()):
        assert rids and set(rids) <= set(ids), mut


# ---- the proj + MLP launch: proj_mlp.hpp launch_proj_mlp / proj_mlp_dispatch ---------------------------------------------------------------------------
PROJ_EDGES = (1, 31, 32, 33, 127, 128, 129)                                 # row counts around one wave's 32-token tile and the 128-row workgroup
PROJ_TAG = 'cvmi_note_kernel("proj_mlp_kernel<%d, %d>", C, VAR);'


def proj_source(csrc=CSRC):
    return open(os.path.join(csrc, "proj_mlp.hpp")).read()


def proj_instances(text):
    """Tags of every instance proj_mlp.hpp can launch, from the call sites of launch_proj_mlp<C, VAR>."""
    return ["proj_mlp_kernel<%s, %s>" % m for m in re.findall(r"return launch_proj_mlp<(\d+), (\d)>\(", text)]


def proj_gaps(text, rows=PROJ_ROWS):
    """What PROJ_ROWS leaves uncovered of the proj + MLP launch, as a list of strings (empty = complete)."""
    gaps = [] if PROJ_TAG in text else ["proj_mlp.hpp no longer tags its launch as proj_mlp_kernel<%d, %d>"]
    inst, tags = set(proj_instances(text)), {r["expect"] for r in rows}
    gaps += [f"{t} has no row" for t in sorted(inst - tags)]
    gaps += [f"rows expect {t}, which the sources no longer launch" for t in sorted(tags - inst)]
    for t in sorted(inst & tags):
        mine = [r for r in rows if r["expect"] == t]
        plain = {r["rows"] for r in mine if r["stats_out"] and not r["kinds"] and r["x_ld"] > r["C"] and r["ao_ld"] > r["C"]}
        gaps += [f"{t}: no padded statistics-out row with {n} rows" for n in PROJ_EDGES if n not in plain]
        if not any(not r["stats_out"] for r in mine):
            gaps.append(f"{t}: no row without statistics out")
        if not any(r["x_ld"] == r["C"] and r["ao_ld"] == r["C"] for r in mine):
            gaps.append(f"{t}: no row with tight strides")
        if not any(r["kinds"] for r in mine):
            gaps.append(f"{t}: no kinds row")
    return gaps


def test_every_proj_mlp_instance_is_in_the_matrix():
    text = proj_source()
    inst = proj_instances(text)
    assert len(inst) == 2 and len(set(inst)) == 2, inst                     # the parser still finds the call sites
    assert sorted(inst) == PROJ_INSTANCES == sorted({proj_pick(144), proj_pick(288)})
    assert "if (C == 144) return launch_proj_mlp<144, 1>(" in text and "return launch_proj_mlp<288, 2>(" in text          # proj_pick's rule
    assert proj_gaps(text) == [], proj_gaps(text)


def test_a_new_proj_mlp_instance_or_a_removed_row_is_caught():
    text = proj_source()
    probe = text + "\n  return launch_proj_mlp<288, 0>(d, s);\n"
    assert proj_gaps(probe) == ["proj_mlp_kernel<288, 0> has no row"]
    probe = text.replace("return launch_proj_mlp<288, 2>(", "return launch_proj_mlp<288, 0>(")
    assert probe != text and proj_gaps(probe) == ["proj_mlp_kernel<288, 0> has no row", "rows expect proj_mlp_kernel<288, 2>, which the sources no longer launch"]
    assert proj_gaps(text.replace("cvmi_note_kernel(", "note_off(")) == ["proj_mlp.hpp no longer tags its launch as proj_mlp_kernel<%d, %d>"]
    drop = lambda *rids: proj_gaps(text, [r for r in PROJ_ROWS if r["id"] not in rids])
    assert drop("proj_c144_rows5_ld148", "proj_c288_rows777_ld292") == []   # (no edge: the instances keep their other rows)
    assert drop("proj_c144_rows33_ld148") == ["proj_mlp_kernel<144, 1>: no padded statistics-out row with 33 rows"]
    assert drop("proj_c288_rows1_ld292", "proj_c288_rows128_ld292") == ["proj_mlp_kernel<288, 2>: no padded statistics-out row with 1 rows",
                                                                        "proj_mlp_kernel<288, 2>: no padded statistics-out row with 128 rows"]
    assert drop("proj_c288_rows129_ld292_nostats", "proj_c288_rows391_ld292_nostats") == ["proj_mlp_kernel<288, 2>: no row without statistics out"]
    assert drop("proj_c144_rows391_ld144") == ["proj_mlp_kernel<144, 1>: no row with tight strides"]
    assert drop("proj_c288_rows391_ld292_kinds") == ["proj_mlp_kernel<288, 2>: no kinds row"]
    assert drop(*[r["id"] for r in PROJ_ROWS if r["C"] == 144]) == ["proj_mlp_kernel<144, 1> has no row"]


def test_proj_and_kinds_rows_are_well_formed():
    ids = [r["id"] for r in TOK_ROWS + MLP_ROWS + MLP_KIND_ROWS + PROJ_ROWS]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    for r in PROJ_ROWS:
        C = r["C"]
        assert r["expect"] == proj_pick(C) and r["proj"] and r["dtypes"] == ("f16", "bf16") and r["rows"] <= 1000, r["id"]
        assert (r["x_ld"], r["ao_ld"]) in ((C + 4, C + 8), (C, C)) and r["x_ld"] % 4 == 0 and r["ao_ld"] % 8 == 0, f"{r['id']}: the alignment contract"
        assert not r["kinds"] or (r["rows"] == 391 and r["stats_out"] and r["x_ld"] > C), r["id"]
    for C in (144, 288):
        mine = [r for r in PROJ_ROWS if r["C"] == C]
        assert {r["rows"] for r in mine if r["stats_out"] and not r["kinds"] and r["x_ld"] > C} >= set(MLP_ROW_COUNTS), C
        assert {r["rows"] for r in mine if not r["stats_out"]} == {129, 391} and [r["rows"] for r in mine if r["x_ld"] == C] == [391], C
        assert sum(r["kinds"] for r in mine) == 1, C
    assert {(r["C"], r["rows"]) for r in PROJ_ROWS} >= set(PROJ_TODAY)
    assert [r["expect"] for r in MLP_KIND_ROWS] == [mlp_pick(144), mlp_pick(288), mlp_pick(288, "0")] and sorted(r["expect"] for r in MLP_KIND_ROWS) == MLP_INSTANCES
    for r in MLP_KIND_ROWS:
        assert r["kinds"] and r["rows"] == 391 and r["stats_out"] and r["x_ld"] == r["C"] + 4 and r["expect"] == mlp_pick(r["C"], r["pipe"]), r["id"]
    assert not any(r.get("kinds") for r in MLP_ROWS)                         # the measured rows of the plain family are what they were
    assert len(KIND_BLOCKS) == 5 and 391 >= (len(KIND_BLOCKS) + 1) * KIND_ROWS   # five kinds of one wave tile each, and plain rows behind them


# ---- the detector's tail: nms.hip nms_launch / yolo_nms_kernel, vision_ops.hip cvmi_detect_decode -----------------------------------------------------
DETECT_SOURCES =("nms.hip", "vision_ops.hip")
# the text nms_pick / nms_workspace mirror: constant or expression -> what op_matrix holds for it
NMS_TEXT = {
    "constexpr int NMS_LDS_A = %d;" % NMS_LDS_A: "NMS_LDS_A",
    "constexpr int NMS_MAX_A = %d;" % NMS_MAX_A: "NMS_MAX_A",
    "constexpr int NMS_MAX_DET = %d;" % NMS_MAX_DET: "NMS_MAX_DET",
    "constexpr int NMS_MAX_NMS = %d;" % NMS_MAX_NMS: "NMS_MAX_NMS",
    "const int nthr = nall <= %d ? 256 : NMS_THREADS;" % NMS_NTHR_N: "the four-wave threshold",
    "const int n = min(nall, NMS_MAX_NMS);": "the max_nms cap behind the sort",
    "const bool geo_lds = !GK && (size_t)Ps * 8 + (size_t)n * sizeof(Cand) <= (size_t)P * 8;": "the geo_lds expression",
    "struct Cand { float x1, y1, x2, y2, area; };": "sizeof(Cand) = %d" % NMS_CAND_BYTES,
    "return (nb * A * %d + 256 + 15) & ~(size_t)15; }" % NMS_WS_RECORD: "the 28-byte workspace record and its 16-byte rounding",
    "static_assert(sizeof(Cand) + sizeof(float) + sizeof(int) == %d," % NMS_WS_RECORD: "the 28-byte workspace record",
    "const bool gk = A > NMS_LDS_A;": "the GK rule",
    "int P = 1024;\n  while (P < A) P <<= 1;": "P",
    "int Ps = 1;\n  while (Ps < nall) Ps <<= 1;": "Ps",
    "max_det > 0 && max_det <= NMS_MAX_DET": "the max_det check",
}
DETECT_TAGS = {"nms.hip": 'cvmi_note_kernel(gk ? "yolo_nms_kernel<true>" : "yolo_nms_kernel<false>");',
               "vision_ops.hip": 'cvmi_note_kernel("detect_decode_kernel<%s>", dtype == CVMI_F16 ? CVMI_F16NAME : "float");'}
NMS_COMBOS = [(False, 256, True), (False, 1024, True), (False, 256, False), (False, 1024, False), (True, 256, False), (True, 1024, False)]


def detect_sources(csrc=CSRC):
    return {name: open(os.path.join(csrc, name)).read() for name in DETECT_SOURCES}


def detect_gaps(sources, nms_rows=NMS_ROWS, decode_rows=DECODE_ROWS):
    """What the detector-tail matrix leaves uncovered, as a list of strings (empty = complete)."""
    gaps = [f"nms.hip no longer reads {text!r} ({what}): nms_pick mirrors something else" for text, what in NMS_TEXT.items() if text not in sources["nms.hip"]]
    gaps += [f"{name} no longer tags its launch with {text}" for name, text in DETECT_TAGS.items() if text not in sources[name]]
    have = {(r["gk"], r["nthr"], r["geo_lds"]) for r in nms_rows}
    gaps += ["yolo_nms_kernel (gk, nthr, geo_lds) = (%s, %d, %s) has no row" % c for c in NMS_COMBOS if c not in have]
    gaps += [f"yolo_nms_kernel: no row with n = {n}" for n in NMS_N_EDGES if not any(r["n"] == n for r in nms_rows)]
    gaps += [f"yolo_nms_kernel: no row with A = {a}" for a in NMS_A_EDGES if not any(r["A"] == a for r in nms_rows)]
    for P in (1024, 16384):
        for n, what in ((P // 4, "P / 4"), (P // 4 + 1, "P / 4 + 1"), (P, "A = P")):
            if not any(r["P"] == P and r["n"] == n and not r["gk"] and (n < P or r["A"] == P) for r in nms_rows):
                gaps.append(f"yolo_nms_kernel: no row with n = {what} at P = {P}")
    checks = (("a GK row with B * A odd", lambda r: r["gk"] and (r["B"] * r["A"]) % 2 == 1), ("a row with B = 1", lambda r: r["B"] == 1),
              ("a cvmi_yolo_nms row with B * A > 4096 * 256", lambda r: r["entry"] == "both" and r["B"] * r["A"] > 4096 * 256),
              ("max_det = 1", lambda r: r["max_det"] == 1), ("max_det = 300 with exactly 300 survivors", lambda r: r["max_det"] == 300 and r["survivors"] == "==300"),
              ("max_det = 300 with more survivors", lambda r: r["max_det"] == 300 and r["survivors"] == ">300"),
              ("max_det = NMS_MAX_DET with more survivors", lambda r: r["max_det"] == NMS_MAX_DET and r["survivors"] == ">%d" % NMS_MAX_DET),
              ("conf_thres = 0", lambda r: r["conf"] == 0), ("iou_thres = 0 with touching boxes", lambda r: r["iou"] == 0 and r["kind"] == "touch"),
              ("iou_thres < 0", lambda r: r["iou"] < 0 and not r["zero"]), ("exact duplicates", lambda r: r["jitter"] == 0 and not r["zero"] and r["kind"] == "cluster"),
              ("duplicated zero-area boxes", lambda r: r["zero"] > 0 and r["jitter"] == 0), ("score ties across the candidate set", lambda r: r["equal_scores"]),
              ("class 61 at max_wh = 7680", lambda r: r["kind"] == "clsoff" and r["nc"] == 62 and r["max_wh"] == 7680.0),
              ("the rounding pairs", lambda r: r["kind"] == "rounding"), ("more candidates than NMS_MAX_NMS", lambda r: r["kind"] == "maxnms" and r["n"] > NMS_MAX_NMS + 100))
    gaps += [f"yolo_nms_kernel: no row with {what}" for what, f in checks if not any(f(r) for r in nms_rows)]
    for dt in ("f16", "f32"):
        mine = [r for r in decode_rows if dt in r["dtypes"]]
        if not mine:
            gaps.append(f"{decode_tag(dt)} has no row")
        gaps += [f"{decode_tag(dt)}: no row with nc = {nc}" for nc in (1, 7, 8, 62, 80, DECODE_NC_MAX[dt]) if not any(r["nc"] == nc for r in mine)]
        gaps += [f"{decode_tag(dt)}: no row with {nl} level(s)" for nl in (1, 2, 3) if not any(len(r["levels"]) == nl for r in mine)]
        for what, f in (("B * A = 1", lambda r: r["B"] * r["A"] == 1), ("B * A = 64", lambda r: r["B"] * r["A"] == 64), ("B * A % 64 != 0", lambda r: r["B"] * r["A"] % 64),
                        ("box_ld > 64", lambda r: r["box_extra"] > 0), ("cls_ld past the padded classes", lambda r: r["cls_extra"] > 0),
                        ("the optional outputs", lambda r: r["optional"]), ("best-class ties", lambda r: r["kind"] == "ties"), ("saturated logits", lambda r: r["kind"] == "saturated"),
                        ("the decode -> NMS chain", lambda r: r["chain"]), ("every seam inside a workgroup", lambda r: set(r["straddle"]) == {"image", "level1", "level2"})):
            if not any(f(r) for r in mine):
                gaps.append(f"{decode_tag(dt)}: no row with {what}")
    return gaps


def test_nms_pick_mirrors_nms_launch_and_the_kernel():
    src = detect_sources()
    assert detect_gaps(src) == [], detect_gaps(src)
    assert nms_pick(1, 0) == (False, 1024, 1, 256, True) and nms_pick(1024, 1024) == (False, 1024, 1024, 256, False)
    assert nms_pick(1024, 256)[4] and not nms_pick(1024, 257)[4] and nms_pick(16384, 4096)[4] and not nms_pick(16384, 4097)[4]
    assert nms_pick(2049, 2048)[3] == 256 and nms_pick(2049, 2049)[3] == 1024
    assert nms_pick(16384, 100)[0] is False and nms_pick(16385, 100)[:2] == (True, 32768) and nms_pick(65536, 65536)[1:3] == (65536, 65536)
    for P in (1024, 2048, 4096, 8192, 16384):                              # without GK the geometry fits behind the keys exactly up to n = P / 4
        assert all(nms_pick(P, n)[4] == (n <= P // 4) for n in range(0, P + 1, 1 if P == 1024 else 61)) and nms_pick(P, P // 4 + 1)[4] is False
    assert nms_workspace(3, 16385) % 16 == 0 and (3 * 16385 * NMS_WS_RECORD + 256) % 16 != 0 and nms_workspace(1, 1) == 288
    assert NMS_CAND_BYTES + 8 == NMS_WS_RECORD
    assert {(g, t, l) for g in (False, True) for t in (256, 1024) for l in (False, True) if not (g and l)} == set(NMS_COMBOS)


def test_detect_rows_are_well_formed():
    ids = [r["id"] for r in NMS_ROWS] + [r["id"] for r in DECODE_ROWS]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    for r in NMS_ROWS:
        assert (r["gk"], r["P"], r["Ps"], r["nthr"], r["geo_lds"]) == nms_pick(r["A"], r["n"]) and r["expect"] == nms_tag(r["A"] > NMS_LDS_A), r["id"]
        assert 0 <= r["n"] <= r["A"] <= NMS_MAX_A and 0 < r["max_det"] <= NMS_MAX_DET and r["conf"] >= 0 and r["kind"] in NMS_KINDS and r["entry"] in ("best", "both"), r["id"]
        assert r["B"] * (4 + r["nc"]) * r["A"] * 4 <= 32 << 20, f"{r['id']}: the input stays under 32 MiB"
    assert sum(r["entry"] == "both" for r in NMS_ROWS) >= 10
    assert any(c["max_det"] == NMS_MAX_DET + 1 for c in NMS_REFUSED)
    for r in DECODE_ROWS:
        assert set(r["dtypes"]) <= {"f16", "f32"} and r["kind"] in ("rand", "ties", "saturated") and 1 <= len(r["levels"]) <= 3, r["id"]
        assert all(r["nc"] <= DECODE_NC_MAX[dt] and r["box_extra"] % 8 == 0 and r["cls_extra"] % 8 == 0 for dt in r["dtypes"]), r["id"]
    for dt, vec in (("f16", 8), ("f32", 4)):                               # the LDS tile: 64 rows of ncp + 1 floats in 64 KiB
        ncp = lambda nc: (nc + vec - 1) // vec * vec
        assert 64 * (ncp(DECODE_NC_MAX[dt]) + 1) * 4 <= 65536 < 64 * (ncp(DECODE_NC_MAX[dt] + 1) + 1) * 4
        assert any(c["dt"] == dt and c["nc"] == DECODE_NC_MAX[dt] + 1 for c in DECODE_REFUSED)
    assert {c.get("best") for c in DECODE_REFUSED} >= {"score", "cls"}
    vis = detect_sources()["vision_ops.hip"]
    assert "const size_t lds = (size_t)64 * (ncp + 1) * sizeof(float);" in vis and 'CVMI_CHECK(lds <= 64 * 1024, "detect_decode: nc too large for the LDS tile");' in vis


def test_a_removed_detect_row_or_a_moved_threshold_is_caught():
    src = detect_sources()
    drop = lambda *rids: detect_gaps(src, nms_rows=[r for r in NMS_ROWS if r["id"] not in rids])
    assert drop("lds_1024_nogeo") == [] and "yolo_nms_kernel (gk, nthr, geo_lds) = (False, 1024, False) has no row" in drop("lds_1024_nogeo", "n4097_quarter_p16384_plus1", "full_16384", "md4096_more")
    assert drop("lds_1024_geo", "n2049_geo", "n4096_quarter_p16384")[0] == "yolo_nms_kernel (gk, nthr, geo_lds) = (False, 1024, True) has no row"
    assert drop("gk_1024_b1", "max_nms")[0] == "yolo_nms_kernel (gk, nthr, geo_lds) = (True, 1024, False) has no row"
    assert drop("n2048") == ["yolo_nms_kernel: no row with n = 2048"]
    assert drop("n257_quarter_p1024_plus1") == ["yolo_nms_kernel: no row with n = 257", "yolo_nms_kernel: no row with n = P / 4 + 1 at P = 1024"]
    assert drop("n4096_quarter_p16384") == ["yolo_nms_kernel: no row with n = P / 4 at P = 16384"]
    assert drop("full_16384") == ["yolo_nms_kernel: no row with A = 16384", "yolo_nms_kernel: no row with n = A = P at P = 16384"]
    assert drop("gk_256_odd") == ["yolo_nms_kernel: no row with A = 16385", "yolo_nms_kernel: no row with a GK row with B * A odd"]
    assert drop("md4096_more") == ["yolo_nms_kernel: no row with max_det = NMS_MAX_DET with more survivors"]
    assert drop("max_nms") == ["yolo_nms_kernel: no row with more candidates than NMS_MAX_NMS"]
    assert drop("rounding") == ["yolo_nms_kernel: no row with the rounding pairs"]
    assert drop("a65536_second_grid_pass") == ["yolo_nms_kernel: no row with a cvmi_yolo_nms row with B * A > 4096 * 256"]
    ddrop = lambda rid: detect_gaps(src, decode_rows=[r for r in DECODE_ROWS if r["id"] != rid])
    assert ddrop("l3_ncmax_f32") == ["detect_decode_kernel<float>: no row with nc = 252"]
    assert ddrop("l1_1") == [f"detect_decode_kernel<{t}>: no row with {w}" for t in ("_Float16", "float") for w in ("nc = 1", "B * A = 1")]
    assert ddrop("saturated") == [f"detect_decode_kernel<{t}>: no row with saturated logits" for t in ("_Float16", "float")]
    probe = dict(src)
    probe["nms.hip"] = src["nms.hip"].replace("nall <= 2048 ? 256", "nall <= 4096 ? 256")
    assert len(detect_gaps(probe)) == 1 and "the four-wave threshold" in detect_gaps(probe)[0]
    probe["nms.hip"] = src["nms.hip"].replace("constexpr int NMS_MAX_NMS = 30000;", "constexpr int NMS_MAX_NMS = 32768;")
    assert len(detect_gaps(probe)) == 1 and "NMS_MAX_NMS" in detect_gaps(probe)[0]
    for name, text in DETECT_TAGS.items():
        probe = dict(src)
        probe[name] = src[name].replace(text, "")
        assert detect_gaps(probe) == [f"{name} no longer tags its launch with {text}"]


# ---- the resampling kernels: resample.hip cvmi_sam2_transform* and the bilinear mask return -----------------------------------------------------
RESAMPLE_ENTRY_RE = r"cvmi_sam2_transform\w*|cvmi_mask_postprocess\w*|cvmi_bilinear_f32|cvmi_mask_extent"
RESAMPLE_TYPES = {"f16": ("f16", "bf16"), "float": ("f32",), "_Float16": ("f16",), "__bf16": ("bf16",)}     # f16: a dual build's operand type (none today)
RESAMPLE_CAP_KIND = {"cvmi_bilinear_f32": "bilinear", "cvmi_mask_postprocess": "bilinear", "cvmi_mask_postprocess_sizes": "bilinear",
                     "cvmi_mask_postprocess_rects_dev": "bilinear", "cvmi_mask_extent": "mask_extent"}       # every other entry: "transform"


def resample_entries(text):
    """{entry: (dual built, body)} of every extern "C" definition in resample.hip whose name matches RESAMPLE_ENTRY_RE (prototypes are skipped)."""
    out = {}
    for m in re.finditer(r'extern "C" int (CVMI_ENTRY\()?(cvmi_\w+)\)?\(([^{;]*)\)\s*(\{|;)', text):
        if m.group(4) == "{" and re.fullmatch(RESAMPLE_ENTRY_RE, m.group(2)):
            out[m.group(2)] = (bool(m.group(1)), text[m.end():text.index("\n}\n", m.end())])
    return out


def resample_constants(text):
    """(AA_MAXTAPS, RECT_MAX, {entry: work items of one pass of each capped grid it launches}) as resample.hip states them."""
    taps = int(re.search(r"constexpr int AA_MAXTAPS = (\d+);", text).group(1))
    rect = int(re.search(r"constexpr int RECT_MAX = (\d+);", text).group(1))
    block, a, b = (int(v) for v in re.search(r"inline int grid_for\(long long total, int block = (\d+), int cap = (\d+) \* (\d+)\)", text).groups())
    caps = {}
    for name, (_, body) in resample_entries(text).items():
        found = set()
        for args in re.findall(r"grid_for\(((?:[^()]|\([^()]*\))*)\)", body):
            parts = [p.strip() for p in re.split(r",(?![^()]*\))", args)]
            found.add((int(parts[2]) if len(parts) > 2 else a * b) * (int(parts[1]) if len(parts) > 1 else block))
        caps[name] = found
    return taps, rect, caps


def _refuses(row, form):
    """Is the row's call through `form` one the entry point must refuse (transform rows: per form; mask-return rows: the whole row)?"""
    ref = row.get("refuse")
    return form in ref if isinstance(ref, dict) else bool(ref)


def resample_gaps(text, rows=RESAMPLE_ROWS):
    """What the resampling matrix leaves uncovered or mirrors wrongly, as a list of strings (empty = complete)."""
    gaps = []
    taps, rect, caps = resample_constants(text)
    if taps != AA_MAXTAPS:
        gaps.append(f"AA_MAXTAPS is {taps} in resample.hip, op_matrix mirrors {AA_MAXTAPS}")
    if rect != RECT_MAX:
        gaps.append(f"RECT_MAX is {rect} in resample.hip, op_matrix mirrors {RECT_MAX}")
    entries = resample_entries(text)
    form_of = {e: f for f, e in list(TRANSFORM_ENTRY.items()) + list(MASK_ENTRY.items())}
    macro = re.search(r"#define LAUNCH_TRANSFORM\(kernel,(?:[^\n]*\\\n)*[^\n]*\n", text)
    launcher_types = re.findall(r"hipLaunchKernelGGL\(kernel<([\w ]+)>", macro.group(0)) if macro else []
    gaps += [f"op_matrix names {e}, which resample.hip no longer defines" for e in sorted(set(form_of) - set(entries))]

    def launched(name, seen=()):
        """Output-type instances an entry launches, through the entry it forwards to if it has no launch of its own."""
        dual, body = entries[name]
        inst = [(k, t, dual) for k, t in re.findall(r"hipLaunchKernelGGL\(\(?(sam2_transform\w*_kernel)<([\w ]+)>", body)]
        inst += [(k, t, dual) for k in re.findall(r"LAUNCH_TRANSFORM\((sam2_transform\w*_kernel),", body) for t in launcher_types]      # the three-type launcher
        fwd = re.search(r"return (cvmi_\w+)\(", body)
        return inst or (launched(fwd.group(1), seen + (name,)) if fwd and fwd.group(1) in entries and fwd.group(1) not in seen else [])

    for name in sorted(entries):
        kind = RESAMPLE_CAP_KIND.get(name, "transform")
        want = {RESAMPLE_GRID_CAP[kind]}
        if caps[name] and caps[name] != want:
            gaps.append(f"{name} caps a grid at {sorted(caps[name])} work items, op_matrix.RESAMPLE_GRID_CAP[{kind!r}] mirrors {sorted(want)}")
        form = form_of.get(name)
        mine = [r for r in rows if form in r["forms"] and not _refuses(r, form)] if form else []
        if not mine:
            gaps.append(f"{name} has no rows in op_matrix.RESAMPLE_ROWS")
            continue
        if form in TRANSFORM_ENTRY:
            inst = launched(name)
            if not inst:
                gaps.append(f"{name}: no sam2_transform kernel launch found")
            for kernel, t, dual in inst:
                for dt in (RESAMPLE_TYPES[t] if dual or t != "f16" else ("f16",)):
                    if not any(dt in r["dtypes"] for r in mine):
                        gaps.append(f"{name}: {kernel}<{t}> ({dt}) has no row that launches it")
            if not any(form in r["forms"] and _refuses(r, form) for r in rows):
                gaps.append(f"{name} has no refused row")
    return gaps


def _resample_hip():
    return open(os.path.join(CSRC, "resample.hip")).read()


def test_resample_rows_mirror_resample_hip_and_cover_every_entry_and_type_instance():
    text = _resample_hip()
    entries = resample_entries(text)
    assert set(entries) == set(TRANSFORM_ENTRY.values()) | set(MASK_ENTRY.values()), sorted(entries)       # the parser still finds the ten entry points
    # no resampling entry is dual-built: the file is compiled once, every kernel instantiated for the three output types in that one build
    assert not [e for e, (dual, _) in entries.items() if dual] and "CVMI_ENTRY" not in text and "CVMI_OPERAND_BF16" not in text and "_bf16(" not in text
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"\bresample\.o\b", makefile) and "resample_bf16.o" not in makefile
    others = "".join(open(p).read() for p in glob.glob(os.path.join(CSRC, "*.hip")) if os.path.basename(p) != "resample.hip")
    assert not re.search(r'extern "C" int (?:CVMI_ENTRY\()?(?:%s)\)?\(' % RESAMPLE_ENTRY_RE, others)           # ... and no other file defines or forwards one
    taps, rect, caps = resample_constants(text)
    assert (taps, rect) == (AA_MAXTAPS, RECT_MAX) == (24, 64)
    assert caps["cvmi_sam2_transform_batch"] == {RESAMPLE_GRID_CAP["transform"]} == {4096 * 256} and caps["cvmi_sam2_transform"] == set()
    assert caps["cvmi_mask_postprocess_rects_dev"] == {RESAMPLE_GRID_CAP["bilinear"]} == {1024 * 256} and caps["cvmi_mask_extent"] == {RESAMPLE_GRID_CAP["mask_extent"]} == {32 * 256}
    assert resample_gaps(text) == [], resample_gaps(text)
    # every entry launches all three output types: every one of them is a (form, type) some row runs
    for form in ("single", "batch", "rects", "rects_dev", "srcs"):
        have = {dt for r in RESAMPLE_ROWS if form in r["forms"] and not _refuses(r, form) for dt in r["dtypes"]}
        assert have == {"f16", "bf16", "f32"}, (form, have)


def test_a_new_resampling_entry_a_removed_row_or_a_moved_constant_is_caught():
    text = _resample_hip()
    probe = text + '\nextern "C" int cvmi_sam2_transform_foo(const uint8_t* src, void* dst, cvmi_stream_t stream_) {\n  return 0;\n}\n'
    assert resample_gaps(probe) == ["cvmi_sam2_transform_foo has no rows in op_matrix.RESAMPLE_ROWS"]
    probe = text + '\nextern "C" int cvmi_mask_postprocess_foo(const float* x) {\n  return 0;\n}\n'
    assert resample_gaps(probe) == ["cvmi_mask_postprocess_foo has no rows in op_matrix.RESAMPLE_ROWS"]
    assert resample_gaps(text + '\nextern "C" int cvmi_sam2_transform_foo(const uint8_t* src);\n') == []              # a prototype is no entry point
    drop = lambda pred: resample_gaps(text, [r for r in RESAMPLE_ROWS if not pred(r)])
    assert drop(lambda r: "mask_extent" in r["forms"]) == ["cvmi_mask_extent has no rows in op_matrix.RESAMPLE_ROWS"]
    strip = lambda form: resample_gaps(text, [dict(r, forms=tuple(f for f in r["forms"] if f != form)) for r in RESAMPLE_ROWS])
    assert strip("mask_postprocess_rects_dev") == ["cvmi_mask_postprocess_rects_dev has no rows in op_matrix.RESAMPLE_ROWS"]
    assert strip("single") == ["cvmi_sam2_transform has no rows in op_matrix.RESAMPLE_ROWS"]
    assert strip("rects_dev") == ["cvmi_sam2_transform_rects_dev has no rows in op_matrix.RESAMPLE_ROWS"]
    unrefused = [dict(r, refuse={f: t for f, t in r["refuse"].items() if f != "srcs"}) if isinstance(r.get("refuse"), dict) else r for r in RESAMPLE_ROWS]
    assert resample_gaps(text, unrefused) == ["cvmi_sam2_transform_srcs has no refused row"]
    def no_bf16(form):                                                         # the form's rows lose bf16; their other forms keep it
        rows = []
        for r in RESAMPLE_ROWS:
            if form in r["forms"]:
                rows += [dict(r, forms=tuple(f for f in r["forms"] if f != form)), dict(r, forms=(form,), dtypes=tuple(d for d in r["dtypes"] if d != "bf16"))]
            else:
                rows.append(r)
        return resample_gaps(text, rows)

    assert no_bf16("srcs") == ["cvmi_sam2_transform_srcs: sam2_transform_srcs_kernel<__bf16> (bf16) has no row that launches it"]
    assert no_bf16("rects") == ["cvmi_sam2_transform_rects: sam2_transform_rects_kernel<__bf16> (bf16) has no row that launches it"]
    assert resample_gaps(text.replace("constexpr int AA_MAXTAPS = 24;", "constexpr int AA_MAXTAPS = 32;")) == ["AA_MAXTAPS is 32 in resample.hip, op_matrix mirrors 24"]
    assert resample_gaps(text.replace("constexpr int RECT_MAX = 64;", "constexpr int RECT_MAX = 128;")) == ["RECT_MAX is 128 in resample.hip, op_matrix mirrors 64"]
    moved = text.replace("int cap = 256 * 16)", "int cap = 256 * 32)")
    assert moved != text and any("cvmi_sam2_transform_srcs caps a grid at [2097152] work items" in g for g in resample_gaps(moved))
    moved = text.replace("grid_for((long long)H * W, 256, 32)", "grid_for((long long)H * W, 256, 64)")
    assert moved != text and resample_gaps(moved) == ["cvmi_mask_extent caps a grid at [16384] work items, op_matrix.RESAMPLE_GRID_CAP['mask_extent'] mirrors [8192]"]


# ---- the contour stage of wire_ops.hip: cvmi_external_contours, cvmi_node_prepare ----------------------------------------------------------------
CONTOUR_RULE_TEXT = ("maxwords = std::max(maxwords, g.H[n] * ((g.W[n] + 31) / 32));", "const size_t lds = (size_t)maxwords * 4;", "const int use_lds = lds <= kLdsMax;",
                     "const size_t dyn = use_lds ? lds : 0;")
CONTOUR_SHAPE_TEXT = {                             # launch shapes the rows were sized for -> how often wire_ops.hip states them
    "template <bool WRITE>\n__global__ __launch_bounds__(%d) void trace_kernel(" % TRACE_LANES: 1,
    "for (int k = threadIdx.x; k < cnt; k += blockDim.x) {": 1,
    "const int y = blockIdx.x * %d + (threadIdx.x >> 6), lane = threadIdx.x & 63;" % ROOT_ROWS_PER_BLOCK: 2,
    "b256(256), grow(cdiv(mh, %d), N);" % ROOT_ROWS_PER_BLOCK: 1,
    "for (int x0 = 0; x0 < t.W; x0 += %d) {" % BALLOT_LANES: 1,
    "inline int grid_for(long long total, int block = 256, int cap = %d) {" % (CONTOUR_GRID_CAP // 256): 1,
}


def _product(expr):
    out = 1
    for f in expr.split("*"):
        out *= int(f)
    return out


def contour_constants(text):
    """(PLANE_MAX, kLdsMax, the opt-in threshold, (the lds tag format, the global tag format)) as wire_ops.hip states them."""
    plane_max = int(re.search(r"constexpr int PLANE_MAX = (\d+);", text).group(1))
    lds_max = _product(re.search(r"constexpr size_t kLdsMax = ([\d *]+);", text).group(1))
    optin = _product(re.search(r"if \(dyn > ([\d *]+)\) \{\s*CVMI_HIP\(hipFuncSetAttribute\(", text).group(1))
    tags = re.search(r'cvmi_note_kernel\(use_lds \? "([^"]*)" : "([^"]*)", \(int\)dyn\);', text)
    return plane_max, lds_max, optin, tags.groups() if tags else ()


def contour_gaps(text, rows=CONTOUR_ROWS, prepare_rows=PREPARE_ROWS):
    """What the contour matrix leaves uncovered, as a list of strings (empty = complete)."""
    plane_max, lds_max, optin, tags = contour_constants(text)
    gaps = []
    for name, got, mirror in (("PLANE_MAX", plane_max, PLANE_MAX), ("kLdsMax", lds_max, TRACE_LDS_MAX), ("the LDS opt-in threshold", optin, TRACE_LDS_OPTIN)):
        if got != mirror:
            gaps.append(f"{name} is {got} in wire_ops.hip, op_matrix mirrors {mirror}")
    gaps += [f"wire_ops.hip no longer states `{t}`" for t in CONTOUR_RULE_TEXT if t not in text]
    gaps += [f"wire_ops.hip states `{t.strip()}` {text.count(t)} times, not {n}" for t, n in CONTOUR_SHAPE_TEXT.items() if text.count(t) != n]
    if tags != ("trace_kernel<lds, %d>", "trace_kernel<global, %d>"):
        gaps.append(f"cvmi_external_contours tags its trace as {tags}, not as trace_kernel<lds, %d> / trace_kernel<global, %d>")
    shapes = {r["id"]: [plane_shape(s) for s in r["planes"]] for r in rows}
    need = {r["id"]: trace_lds_bytes(shapes[r["id"]]) for r in rows}
    for r in rows:                                                          # the source's rule, with the source's constant, on the row's shapes
        if contour_tag(shapes[r["id"]], lds_max) != r["expect"]:
            gaps.append(f"row {r['id']} expects {r['expect']}, the rule of wire_ops.hip gives {contour_tag(shapes[r['id']], lds_max)}")
    for name, T in (("the LDS opt-in threshold", optin), ("kLdsMax", lds_max)):
        if not any(b == T for b in need.values()):
            gaps.append(f"{name}: no row whose largest plane needs exactly {T} bytes")
        if not any(T < b <= T + 8 for b in need.values()):
            gaps.append(f"{name}: no row whose largest plane needs one or two words more than {T} bytes")
        if not any(b < T for b in need.values()):
            gaps.append(f"{name}: no row below {T} bytes")
    fams = {re.match(r"trace_kernel<(\w+),", r["expect"]).group(1) for r in rows}
    gaps += [f"the tag {t} is expected by no row" for t in tags if re.match(r"trace_kernel<(\w+),", t).group(1) not in fams]
    for r in rows:                                                          # one large plane moves every plane of the call: the path rows carry small planes too
        if need[r["id"]] > min(optin, lds_max) - 8 and not any(h * w <= 9 * 129 for h, w in shapes[r["id"]]):
            gaps.append(f"row {r['id']} reaches a threshold without a small plane in the same call")
    if not any(len(s) > plane_max for s in shapes.values()):
        gaps.append(f"no contour row with more than PLANE_MAX = {plane_max} planes")
    if not any(len(r["planes"]) > plane_max and [b for b in r["boxes"][plane_max - 1:] if b != "none"] and set(r["boxes"][:plane_max - 1]) == {"none"} for r in prepare_rows):
        gaps.append(f"no prepare row with boxes only on plane {plane_max - 1} and after it")
    if not any(h * w > CONTOUR_GRID_CAP for s in shapes.values() for h, w in s):
        gaps.append(f"no contour row with a plane of more than {CONTOUR_GRID_CAP} pixels")
    if not any(h * w > CONTOUR_GRID_CAP for r in prepare_rows for h, w, _ in r["planes"]):
        gaps.append(f"no prepare row with a plane of more than {CONTOUR_GRID_CAP} pixels")
    if not any(s[0] == "lattice" and ((s[1] + 1) // 2) * ((s[2] + 1) // 2) > TRACE_LANES and (s[2] + 1) // 2 > BALLOT_LANES and s[1] > ROOT_ROWS_PER_BLOCK
               for r in rows for s in r["planes"]):
        gaps.append("no lattice plane with more contours than trace lanes, more roots in a row than ballot lanes and more rows than one root block")
    return gaps


def _wire_ops():
    return open(os.path.join(CSRC, "wire_ops.hip")).read()


def test_contour_rows_mirror_wire_ops_and_cover_every_trace_path_and_threshold():
    text = _wire_ops()
    assert contour_constants(text) == (32, 160 * 1024, 64 * 1024, ("trace_kernel<lds, %d>", "trace_kernel<global, %d>"))      # the parser still finds them
    assert (PLANE_MAX, TRACE_LDS_MAX, TRACE_LDS_OPTIN, CONTOUR_GRID_CAP) == (32, 163840, 65536, 1024 * 256)
    assert contour_gaps(text) == [], contour_gaps(text)
    ids = [r["id"] for r in CONTOUR_ROWS] + [CONTOUR_CAPACITY_ROW["id"]]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    for r in CONTOUR_ROWS + [CONTOUR_CAPACITY_ROW]:
        assert r["expect"] == contour_tag([plane_shape(s) for s in r["planes"]]), r["id"]
    by = {r["id"]: r for r in CONTOUR_ROWS}
    assert [by[i]["expect"] for i in ("lds_64k_no_optin", "lds_64k_plus_optin", "lds_160k_exact", "global_160k_plus", "global_40961x2")] == \
        ["trace_kernel<lds, 65536>", "trace_kernel<lds, 65540>", "trace_kernel<lds, 163840>", "trace_kernel<global, 0>", "trace_kernel<global, 0>"]
    # probes, as the sibling guards do: a moved constant, a moved rule, a removed row
    moved = text.replace("constexpr size_t kLdsMax = 160 * 1024;", "constexpr size_t kLdsMax = 192 * 1024;")
    g = contour_gaps(moved)
    assert moved != text and "kLdsMax is 196608 in wire_ops.hip, op_matrix mirrors 163840" in g and "kLdsMax: no row whose largest plane needs exactly 196608 bytes" in g \
        and "row global_160k_plus expects trace_kernel<global, 0>, the rule of wire_ops.hip gives trace_kernel<lds, 163844>" in g \
        and "the tag trace_kernel<global, %d> is expected by no row" not in g, g
    moved = text.replace("if (dyn > 64 * 1024) {", "if (dyn > 96 * 1024) {")
    assert moved != text and contour_gaps(moved) == ["the LDS opt-in threshold is 98304 in wire_ops.hip, op_matrix mirrors 65536",
                                                     "the LDS opt-in threshold: no row whose largest plane needs exactly 98304 bytes",
                                                     "the LDS opt-in threshold: no row whose largest plane needs one or two words more than 98304 bytes"]
    moved = text.replace("constexpr int PLANE_MAX = 32;", "constexpr int PLANE_MAX = 128;")
    assert contour_gaps(moved) == ["PLANE_MAX is 128 in wire_ops.hip, op_matrix mirrors 32", "no contour row with more than PLANE_MAX = 128 planes",
                                   "no prepare row with boxes only on plane 127 and after it"]
    moved = text.replace("const int use_lds = lds <= kLdsMax;", "const int use_lds = lds < kLdsMax;")
    assert contour_gaps(moved) == ["wire_ops.hip no longer states `const int use_lds = lds <= kLdsMax;`"]
    moved = text.replace('cvmi_note_kernel(use_lds ? "trace_kernel<lds, %d>"', 'note_off(use_lds ? "trace_kernel<lds, %d>"')
    assert any("tags its trace as ()" in m for m in contour_gaps(moved))
    drop = lambda *rids: contour_gaps(text, [r for r in CONTOUR_ROWS if r["id"] not in rids])
    assert drop("lds_160k_exact") == ["kLdsMax: no row whose largest plane needs exactly 163840 bytes"]
    assert drop("global_160k_plus") == []                                  # (global_40961x2 is one word past kLdsMax too)
    assert drop("global_160k_plus", "global_40961x2") == ["kLdsMax: no row whose largest plane needs one or two words more than 163840 bytes",
                                                          "the tag trace_kernel<global, %d> is expected by no row"]
    assert drop("lds_64k_no_optin") == ["the LDS opt-in threshold: no row whose largest plane needs exactly 65536 bytes"]
    assert drop("lds_64k_plus_optin") == ["the LDS opt-in threshold: no row whose largest plane needs one or two words more than 65536 bytes"]
    assert drop("plane_max_plus_1", "word_edges", *[i for i in by if i.startswith(("lds_", "global_"))])[-1] == "no contour row with more than PLANE_MAX = 32 planes"
    assert drop("grid_stride_513x512") == ["no contour row with a plane of more than 262144 pixels"]
    assert drop("lattice_9x129")[-1].startswith("no lattice plane with more contours than trace lanes")
    assert contour_gaps(text, prepare_rows=[r for r in PREPARE_ROWS if r["id"] != "plane_max_plus_1"]) == ["no prepare row with boxes only on plane 31 and after it"]
    alone = [dict(r, planes=r["planes"][-1:]) if r["id"] == "lds_160k_exact" else r for r in CONTOUR_ROWS]
    assert contour_gaps(text, alone) == ["row lds_160k_exact reaches a threshold without a small plane in the same call"]
