"""tools/check_isa.py --same on hand-written assembly: same / reordered / a replaced instruction / a changed register count"""
import importlib.util
import io
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNEL = """\t.text
\t.type\t_ZN4clfa6k_demoEPf,@function
_ZN4clfa6k_demoEPf: ; @_ZN4clfa6k_demoEPf
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v1, 0
\tv_mov_b32_e32 v2, 1.0 ; a comment
\ts_cbranch_execz .LBB{fn}_2
; %bb.1:
\t{op} v3, v1, v2
.LBB{fn}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel _ZN4clfa6k_demoEPf
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_group_segment_fixed_size 0
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{fn}:
\t.type\t__hip_cuid_{cuid},@object
"""


def _mod():
    spec = importlib.util.spec_from_file_location("check_isa", os.path.join(ROOT, "tools", "check_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _verdict(tmp_path, new_text):
    old = tmp_path / "old.s"
    new = tmp_path / "new.s"
    old.write_text(KERNEL.format(fn=0, op="v_add_f32_e32", vgpr=4, cuid="aa"))
    new.write_text(new_text)
    out = io.StringIO()
    bad = _mod().same(str(old), str(new), out)
    first = out.getvalue().split("\n")[0].split()
    assert first[0] == "_ZN4clfa6k_demoEPf"
    return bad, first[1], first[2]


def test_same_ignores_label_numbers_comments_and_cuid(tmp_path):
    assert _verdict(tmp_path, KERNEL.format(fn=3, op="v_add_f32_e32", vgpr=4, cuid="bb")) == (0, "6", "same")


def test_reordered_within_a_block(tmp_path):
    text = KERNEL.format(fn=0, op="v_add_f32_e32", vgpr=4, cuid="aa")
    a, b = "\tv_mov_b32_e32 v1, 0\n", "\tv_mov_b32_e32 v2, 1.0 ; a comment\n"
    assert _verdict(tmp_path, text.replace(a + b, b + a)) == (0, "6", "reordered")


def test_replaced_instruction_is_different(tmp_path):
    assert _verdict(tmp_path, KERNEL.format(fn=0, op="v_mul_f32_e32", vgpr=4, cuid="aa")) == (1, "6", "DIFFERENT")


def test_changed_register_count_is_different(tmp_path):
    assert _verdict(tmp_path, KERNEL.format(fn=0, op="v_add_f32_e32", vgpr=5, cuid="aa")) == (1, "6", "DIFFERENT")


def test_missing_kernel_counts(tmp_path):
    old = tmp_path / "old.s"
    new = tmp_path / "new.s"
    old.write_text(KERNEL.format(fn=0, op="v_add_f32_e32", vgpr=4, cuid="aa"))
    new.write_text("\t.text\n")
    assert _mod().same(str(old), str(new), io.StringIO()) == 1
