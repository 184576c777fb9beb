"""Inline-assembly hazard lint (tools/isa_lint.py) over the kernels that use asm vector instructions next to MFMAs.

The compiler pads matrix-pipe hazards only for instructions it knows; an asm `v_pk_add_f32` whose result an MFMA reads one
instruction later gives wrong results that depend on register allocation (seen once in round 2).  The lint compiles the
sources to gfx950 assembly (no GPU needed) and fails on any such site, so a scheduling change cannot bring it back unnoticed."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint  # noqa: E402

SNIPPET = """
kern:
	v_mfma_f32_16x16x4_f32 v[170:173], v27, v79, v[170:173]
	;;#ASMSTART
	v_pk_add_f32 v[188:189], v[74:75], v[90:91] neg_lo:[0,1] neg_hi:[0,1]
	;;#ASMEND
	%s
	v_mfma_f32_16x16x4_f32 v[74:77], v12, v188, v[170:173]
.Lfunc_end0:
"""


def test_lint_flags_an_asm_result_consumed_by_the_next_mfma():
    bad = [f for f in isa_lint.lint_text(SNIPPET % "v_mov_b32_e32 v1, v2") if f[2] == "A"]
    assert len(bad) == 1 and "v[188:189]" in bad[0][3]
    assert not [f for f in isa_lint.lint_text(SNIPPET % "s_nop 1") if f[2] == "A"]           # two wait states: fine
    assert not [f for f in isa_lint.lint_text(SNIPPET.replace("v12, v188", "v12, v190") % "") if f[2] == "A"]


LOOP = """
kern:
.LBB0_1:
	v_mfma_f32_16x16x4_f32 v[74:77], v12, v188, v[170:173]
	v_mov_b32_e32 v1, v2
	v_mov_b32_e32 v3, v4
	;;#ASMSTART
	v_pk_add_f32 v[188:189], v[74:75], v[90:91]
	;;#ASMEND
	%s
	s_cbranch_scc1 .LBB0_1
	s_endpgm
.Lfunc_end0:
"""


def test_lint_follows_loop_back_edges():
    """The asm result is consumed by the MFMA at the TOP of the loop, one branch later: invisible in textual order."""
    bad = [f for f in isa_lint.lint_text(LOOP % "") if f[2] == "A"]
    assert len(bad) == 1 and "v[188:189]" in bad[0][3]
    assert not [f for f in isa_lint.lint_text(LOOP % "s_nop 0") if f[2] == "A"]      # s_nop 0 + the branch: two wait states


SOURCES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "*_amd", "csrc", "*.hip")))


@pytest.fixture(scope="module")
def assembly():
    """gfx950 assembly of every csrc/*.hip, compiled once per module (in parallel: ~20 translation units), by file name."""
    from concurrent.futures import ThreadPoolExecutor
    csrc = os.path.dirname(glob.glob(os.path.join(ROOT, "*_amd", "csrc", SOURCES[0]))[0])
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        texts = list(ex.map(lambda n: isa_lint.compile_to_asm(os.path.join(csrc, n)), SOURCES))
    return dict(zip(SOURCES, texts))


def _n_asm(text):
    return sum(1 for fn in isa_lint.parse(text).values() for i in fn if i["asm"] and i["op"].startswith("v_"))


def test_the_lint_sees_every_asm_bearing_kernel(assembly):
    """The set of sources whose assembly holds inline-asm vector instructions is found, not listed by hand: a new kernel with asm
    is linted as soon as it exists.  The four known today must be among them (an empty set would mean the format changed)."""
    bearing = {n for n, t in assembly.items() if _n_asm(t) > 0}
    assert {"conv_bwd16.hip", "conv_mfma.hip", "conv_wino8.hip", "conv_wgrad_wino.hip"} <= bearing, sorted(bearing)


@pytest.mark.parametrize("name", SOURCES)
def test_no_asm_to_mfma_hazard_in_the_kernels(assembly, name):
    text = assembly[name]
    n_asm = _n_asm(text)
    if n_asm:       # an asm-bearing source: the lint must have seen its instructions (a handful would mean a parse problem)
        assert n_asm > 100, "the lint did not see the inline-asm instructions (assembly format changed?)"
    errs = [f for f in isa_lint.lint_text(text) if f[2] == "A"]
    assert not errs, errs[:5]
