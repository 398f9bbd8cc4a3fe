"""tools/isa_cmp.py's normalizer on hand-written assembly (no compile, no GPU)."""
import importlib.util
import io
import os

_spec = importlib.util.spec_from_file_location(
    "isa_cmp", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "isa_cmp.py"))
isa_cmp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_cmp)


def _asm(index, add="v_add_f64 v[0:1], v[0:1], v[2:3]", vgprs=12):
    """A one-kernel assembly file as hipcc lays it out, the kernel being function `index` of its file."""
    return f"""\t.text
\t.globl\tk_demo ; -- Begin function k_demo
\t.p2align\t8
\t.type\tk_demo,@function
k_demo: ; @k_demo
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_cbranch_execz .LBB{index}_2
; %bb.1: ; in Loop: Header=BB{index}_1 Depth=1
\t{add} ; a comment
.LBB{index}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel k_demo
\t\t.amdhsa_next_free_vgpr {vgprs}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{index}:
\t.size\tk_demo, .Lfunc_end{index}-k_demo
amdhsa.kernels:
  - .agpr_count:     0
    .group_segment_fixed_size: 512
    .name:           k_demo
    .private_segment_fixed_size: 0
    .sgpr_count:     10
    .sgpr_spill_count: 0
    .symbol:         k_demo.kd
    .vgpr_count:     {vgprs}
    .vgpr_spill_count: 0
"""


def test_normalize_drops_comments_directives_and_function_index():
    lines = isa_cmp.normalize(_asm(7).split("k_demo: ; @k_demo\n")[1].split(".Lfunc_end")[0])
    assert lines == ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "s_cbranch_execz .LBB_2",
                     "v_add_f64 v[0:1], v[0:1], v[2:3]", ".LBB_2:", "s_endpgm"]


def test_same_body_other_label_index_is_equal():
    a, b = isa_cmp.kernels_of(_asm(2)), isa_cmp.kernels_of(_asm(0))
    assert list(a) == ["k_demo"] and a == b
    assert a["k_demo"]["lines"] == 5 and a["k_demo"]["vgpr"] == 12 and a["k_demo"]["lds"] == 512
    for k in (a, b):
        k["k_demo"]["file"] = "x.s"
    assert isa_cmp.compare(a, b, out=io.StringIO()) == 0


def test_one_changed_instruction_differs():
    a = isa_cmp.kernels_of(_asm(2))
    b = isa_cmp.kernels_of(_asm(2, add="v_add_f64 v[0:1], v[0:1], v[4:5]"))
    assert a["k_demo"]["hash"] != b["k_demo"]["hash"] and a["k_demo"]["lines"] == b["k_demo"]["lines"]
    for k in (a, b):
        k["k_demo"]["file"] = "x.s"
    out = io.StringIO()
    assert isa_cmp.compare(a, b, out=out) == 1 and "DIFFERS" in out.getvalue()


def test_changed_resources_or_missing_kernel_differ():
    a, b = isa_cmp.kernels_of(_asm(2)), isa_cmp.kernels_of(_asm(2, vgprs=16))
    assert a["k_demo"]["hash"] == b["k_demo"]["hash"]
    for k in (a, b):
        k["k_demo"]["file"] = "x.s"
    assert isa_cmp.compare(a, b, out=io.StringIO()) == 1
    out = io.StringIO()
    assert isa_cmp.compare(a, {}, out=out) == 1 and "MISSING" in out.getvalue()
