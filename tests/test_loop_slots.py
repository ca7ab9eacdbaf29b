"""tools/loop_slots.py on a small hand-written assembly sample (tests/golden/loop_slots/sample.s, not
compiler output of the product): the classification by mnemonic prefix, the hot path through the
marked loop (the longest pass that enters no `cold` block, with and without the `opt` block) and the
handling of the marker statements."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
SAMPLE = os.path.join(REPO, "tests", "golden", "loop_slots", "sample.s")


@pytest.fixture(scope="module")
def ls():
    import loop_slots

    return loop_slots


@pytest.mark.parametrize("mn,cls", [
    ("v_fma_f64", "valu_f64"), ("v_cmp_gt_f64_e32", "valu_f64"), ("v_min_f64", "valu_f64"),
    ("v_cndmask_b32_e64", "valu_cndmask"), ("v_mov_b64_e32", "valu_mov"), ("v_mov_b32_e32", "valu_mov"),
    ("v_add_u32_e32", "valu_other"), ("v_readfirstlane_b32", "valu_other"),
    ("s_and_b64", "scalar"), ("s_cselect_b64", "scalar"), ("s_load_dwordx2", "scalar"), ("s_sleep", "scalar"),
    ("s_waitcnt", "wait"), ("s_waitcnt_vscnt", "wait"), ("s_nop", "nop"),
    ("s_branch", "branch"), ("s_cbranch_execz", "branch"), ("s_cbranch_scc1", "branch"), ("s_endpgm", "branch"),
    ("ds_read2_b64", "lds"), ("ds_write_b32", "lds"),
    ("global_load_dwordx4", "vmem"), ("flat_load_dword", "vmem"), ("buffer_load_dword", "vmem"),
    ("scratch_load_dword", "vmem"),
])
def test_classify(ls, mn, cls):
    assert ls.classify(mn) == cls


def test_sample_loop_counts(ls):
    rows = ls.report(open(SAMPLE).read(), "sample")
    assert [(r["loop"], r["occurrence"]) for r in rows] == [("demo", 1)]
    full, skip = rows[0]["full"], rows[0]["skip"]
    # the pass through the opt block, by hand: blocks 2, 3, 4, 5, 1 (the cold block 6 is never entered)
    assert full == {"valu_f64": 5, "valu_cndmask": 1, "valu_mov": 1, "valu_other": 2, "scalar": 2, "lds": 1,
                    "vmem": 0, "wait": 1, "nop": 1, "branch": 4, "valu": 9, "total": 18, "blocks": 5}
    # ... and around it: the rcp, the multiply and the integer add less
    assert skip["total"] == 15 and skip["valu_f64"] == 3 and skip["valu_other"] == 1 and skip["blocks"] == 4
    assert skip["branch"] == full["branch"] and skip["wait"] == 1
    # an instruction inside an asm bracket counts, the marker statements do not
    assert full["valu_f64"] == 5


def test_markers_and_kernel_selection(ls):
    text = open(SAMPLE).read()
    assert ls.report(text, "other") == []          # a kernel without a `begin` marker
    assert len(ls.report(text, "_ZN4d2dk")) == 1   # substring match over every kernel
    bl = ls.blocks(ls.kernels(text)["_ZN4d2dk6sampleEv"])
    marks = sorted(m for b in bl.values() for m in b.marks)
    assert marks == [("begin", "demo"), ("cold", "scan"), ("opt", "extra")]
    # the cold block is longer than every hot one: the longest pass must still avoid it
    cold = next(b for b in bl.values() if ("cold", "scan") in b.marks)
    assert len(cold.ins) > 8 and cold.name not in ls.longest_pass(bl, ".LBB0_2", {cold.name})


def test_hash_ignores_markers(ls):
    text = open(SAMPLE).read()
    bare = re.sub(r"[ \t]*;;#ASMSTART\n[ \t]*; D2D_LOOP[^\n]*\n[ \t]*;;#ASMEND\n", "", text)
    assert "D2D_LOOP" not in bare and "v_min_f64" in bare
    assert ls.body_hashes(text) == ls.body_hashes(bare)
    other = bare.replace("v_rcp_f64_e32 v[10:11]", "v_rcp_f64_e32 v[12:13]")
    assert ls.body_hashes(other)["_ZN4d2dk6sampleEv"] != ls.body_hashes(bare)["_ZN4d2dk6sampleEv"]
    assert ls.body_hashes(other)["_ZN4d2dk5otherEv"] == ls.body_hashes(bare)["_ZN4d2dk5otherEv"]


def test_command_line(tmp_path):
    out = tmp_path / "rows.json"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "loop_slots.py"), SAMPLE, "--kernel", "sample",
                        "--json", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "demo#1" in r.stdout and "full" in r.stdout and "skip" in r.stdout
    import json

    assert json.load(open(out))[0]["full"]["total"] == 18
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "loop_slots.py"), SAMPLE, "--kernel", "other"],
                       capture_output=True, text=True)
    assert r.returncode != 0
