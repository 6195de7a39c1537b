"""tools/isa_diff.py: what it treats as the same kernel and the same code (no compiler, no GPU: two canned snippets)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_diff  # noqa: E402

# the same kernel before and after its tag type left the anonymous namespace: another mangled name, another function number
# in the local labels, another source hash, other comments -- and one resource number per side to tell the sides apart
SNIPPET = """\t.globl\t{sym} ; -- Begin function {sym}
\t.type\t{sym},@function
{sym}: ; @{sym}
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0{pad} ; {comment}
\ts_cbranch_scc1 .LBB{n}_2
.LBB{n}_2: ; in Loop: Header=BB{n}_1 Depth=1
\t{last}
.Lfunc_end{n}:
\t.size\t{sym}, .Lfunc_end{n}-{sym}
\t; -- End function
\t.globl\t__hip_cuid_{cuid}
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           8
    .group_segment_fixed_size: 36864
    .name:           {sym}
    .private_segment_fixed_size: 0
    .sgpr_count:     44
    .sgpr_spill_count: 0
    .vgpr_count:     {vgpr}
    .vgpr_spill_count: 0
...
\t.end_amdgpu_metadata
"""
OLD_SYM, NEW_SYM = "_ZN5peclr12_GLOBAL__N_11kINS0_4BF16EEEvi", "_ZN5peclr12_GLOBAL__N_11kINS_4BF16EEEvi"
DEMANGLED = {OLD_SYM: "void peclr::(anonymous namespace)::k<peclr::(anonymous namespace)::BF16>(int)",
             NEW_SYM: "void peclr::(anonymous namespace)::k<peclr::BF16>(int)"}


def demangle(symbols):
    return {s: DEMANGLED[s] for s in symbols}


def snippet(sym, n, cuid, comment, pad="", last="s_endpgm", vgpr=152):
    return SNIPPET.format(sym=sym, n=n, cuid=cuid, comment=comment, pad=pad, last=last, vgpr=vgpr)


OLD = snippet(OLD_SYM, 0, "be558f393de4b125", "old")


def test_plain_name_drops_namespaces_only():
    assert isa_diff.plain_name(DEMANGLED[OLD_SYM]) == "void k<BF16>(int)"
    assert isa_diff.plain_name(DEMANGLED[NEW_SYM]) == "void k<BF16>(int)"
    assert isa_diff.plain_name("void peclr::(anonymous namespace)::k<peclr::F16>(int)") == "void k<F16>(int)"


def test_renamed_kernel_with_same_code_is_identical():
    new = snippet(NEW_SYM, 3, "0123456789abcdef", "new, other comment", pad="   ")
    verdict, rows, same = isa_diff.compare(OLD, new, demangle)
    assert same and verdict.startswith("identical (1 functions, 1 kernels)")
    assert len(rows) == 1 and "152|152" in rows[0] and "36864|36864" in rows[0] and rows[0].endswith("void k<BF16>(int)")


def test_one_changed_instruction_is_found():
    verdict, rows, same = isa_diff.compare(OLD, snippet(NEW_SYM, 3, "0", "x", last="s_nop 0"), demangle)
    assert not same and verdict.startswith("DIFFERENT: void k<BF16>(int)")
    assert "a: s_endpgm" in verdict and "b: s_nop 0" in verdict


def test_one_changed_resource_number_is_found():
    verdict, rows, same = isa_diff.compare(OLD, snippet(NEW_SYM, 3, "0", "x", vgpr=153), demangle)
    assert not same and verdict.startswith("identical") and rows[0].lstrip().startswith("!=") and "152|153" in rows[0]


# a kernel renamed on purpose (two kernels folded into one template): the names differ after demangling too, so it takes --pair
FOLDED_SYM = "_ZN5peclr12_GLOBAL__N_12k2INS_4BF16ENS0_5ArgsWEEEvi"
FOLDED = dict(DEMANGLED, **{FOLDED_SYM: "void peclr::(anonymous namespace)::k2<peclr::BF16, peclr::(anonymous namespace)::ArgsW>(int)"})
PAIR = [("void k<BF16>(int)", "k2<BF16, ArgsW>")]                       # (NEW as an unambiguous part of the name)


def demangle_folded(symbols):
    return {s: FOLDED[s] for s in symbols}


def test_pair_compares_a_renamed_kernel_with_its_counterpart():
    new = snippet(FOLDED_SYM, 5, "0123456789abcdef", "folded")
    verdict, rows, same = isa_diff.compare(OLD, new, demangle_folded)
    assert not same and verdict.startswith("DIFFERENT function lists")   # unpaired: one-sided on both sides
    verdict, rows, same = isa_diff.compare(OLD, new, demangle_folded, pairs=PAIR)
    assert same and verdict.startswith("identical (1 functions, 1 kernels)")
    assert rows[0] == "  paired: a's void k<BF16>(int) = b's void k2<BF16, ArgsW>(int)"
    assert len(rows) == 2 and "152|152" in rows[1] and rows[1].endswith("void k2<BF16, ArgsW>(int)")


def test_pair_still_finds_a_changed_instruction_and_a_changed_resource():
    verdict, rows, same = isa_diff.compare(OLD, snippet(FOLDED_SYM, 5, "0", "x", last="s_nop 0"), demangle_folded, pairs=PAIR)
    assert not same and verdict.startswith("DIFFERENT: void k2<BF16, ArgsW>(int)")
    assert "a: s_endpgm" in verdict and "b: s_nop 0" in verdict
    verdict, rows, same = isa_diff.compare(OLD, snippet(FOLDED_SYM, 5, "0", "x", vgpr=153), demangle_folded, pairs=PAIR)
    assert not same and verdict.startswith("identical") and rows[1].lstrip().startswith("!=") and "152|153" in rows[1]


def test_unmatched_pair_is_an_error():
    import pytest
    new = snippet(FOLDED_SYM, 5, "0", "x")
    for pairs in ([("void nothing<BF16>(int)", "k2<BF16, ArgsW>")],      # a has no such function
                  [("void k<BF16>(int)", "k3")],                          # b has none
                  PAIR + [("k7", "k8")]):                                 # neither side has
        with pytest.raises(ValueError, match="--pair"):
            isa_diff.compare(OLD, new, demangle_folded, pairs=pairs)
    seen = set()                                                          # (one file of several: left to the caller, who collects)
    assert isa_diff.compare(OLD, new, demangle_folded, pairs=PAIR + [("k7", "k8")], applied=seen)[2] and seen == set(PAIR)


def test_missing_kernel_is_found():
    other = dict(DEMANGLED)
    other[NEW_SYM] = "void peclr::(anonymous namespace)::k<peclr::F16>(int)"
    verdict, rows, same = isa_diff.compare(OLD, snippet(NEW_SYM, 0, "0", "x"), lambda syms: {s: other[s] for s in syms})
    assert not same and verdict.startswith("DIFFERENT function lists")
