"""Static instruction-class counts of one kernel from hipcc's assembly (compile the .hip with the
flags of ar_slam_amd/build.py plus --cuda-device-only -S -gline-tables-only): the whole kernel and,
with a source line range, the instructions the line table attributes to it.
usage: python tools/isa_counts.py file.s kernel_substring [first_line last_line]"""
import collections
import re
import sys


def klass(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "MFMA"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vector memory"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith(("s_load", "s_buffer_load")):
        return "scalar memory"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def main():
    path, kern = sys.argv[1], sys.argv[2]
    lo, hi = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (0, 0)
    whole, stage, detail = collections.Counter(), collections.Counter(), collections.Counter()
    inside, line, name = False, 0, ""
    for t in open(path):
        t = t.strip()
        if not inside:
            m = re.match(r"(\w+):", t)
            if m and kern in m.group(1):
                inside, name = True, m.group(1)
            continue
        t = t.split(";")[0].strip()
        if t.startswith(".Lfunc_end"):
            break
        m = re.match(r"\.loc\s+\d+\s+(\d+)", t)
        if m:
            line = int(m.group(1))
            continue
        if not t or t.startswith((".", ";", "//")) or t.endswith(":"):
            continue
        op = t.split()[0]
        k = klass(op)
        whole[k] += 1
        whole["all"] += 1
        if lo <= line <= hi:
            stage[k] += 1
            stage["all"] += 1
            for pat, label in (("v_mul_lo_u32", "integer multiplies"), ("v_mad_u64_u32", "integer multiplies"),
                               ("v_mad_i64_i32", "integer multiplies"), ("v_mul_hi_u32", "integer multiplies"),
                               ("v_lshl_add_u64", "v_lshl_add_u64"), ("s_cbranch_execz", "s_cbranch_execz"),
                               ("s_and_saveexec_b64", "s_and_saveexec_b64"), ("ds_read_b64", "ds_read_b64"),
                               ("ds_read_b128", "ds_read_b128"), ("global_store", "global stores"), ("buffer_store", "buffer stores"),
                               ("global_load", "global loads")):
                if op.startswith(pat):
                    detail[label] += 1
    order = ["all", "VALU", "MFMA", "LDS", "vector memory", "SALU", "scalar memory", "branch", "s_waitcnt", "other"]
    print(name)
    print("  whole kernel :", ", ".join(f"{k} {whole[k]}" for k in order if whole[k]))
    if hi:
        print(f"  lines {lo}-{hi}:", ", ".join(f"{k} {stage[k]}" for k in order if stage[k]))
        print("    of which   :", ", ".join(f"{k} {v}" for k, v in sorted(detail.items())))


if __name__ == "__main__":
    main()
