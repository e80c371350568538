"""Per-kernel table of the batched-decode passes from a rocprofv3 kernel trace (csv) of

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
        python scripts/batch_bench.py --legs batch --R 8 --reps 1

    python scripts/batch_prof_table.py DIR PASSES [R] > profiles/batch/batch_kernels_R8.md

With R given (a wide pass: scripts/batch_wide_bench.py --R 64 --forms mfma --reps 1) the exact GEMM's
launches are listed per workgroup count, so the few-workgroup GEMMs show as lines of their own.

The process also prefills the slots' prompts; the passes are the launches from the first batch pass on
(two launches before the first k_attn_slots that follows the last prompt's k_rope_kv_prefill).  PASSES =
warm-up + timed passes of that run (8 + 24)."""
import collections
import csv
import glob
import os
import re
import sys


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    m = re.match(r"(?:void )?(?:\w+::)*(\w+)", name)  # without namespaces, template and call arguments
    return m.group(1) if m else name


def workgroups(r):
    n = 1
    for ax in "XYZ":
        n *= int(r["Grid_Size_" + ax]) // max(int(r["Workgroup_Size_" + ax]), 1)
    return n


def main():
    d, passes = sys.argv[1], int(sys.argv[2])
    R = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    path = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    names = [short(r["Kernel_Name"]) for r in rows]
    if len(sys.argv) > 3:
        names = [f"{n} ({workgroups(r)} wg)" if n.startswith("k_gemm_x") else n for r, n in zip(rows, names)]
    last_pf = max(i for i, n in enumerate(names) if n == "k_rope_kv_prefill")
    first = next(i for i in range(last_pf, len(names)) if names[i] == "k_attn_slots") - 2
    rows, names = rows[first:], names[first:]
    tot, cnt = collections.Counter(), collections.Counter()
    for r, n in zip(rows, names):
        tot[n] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        cnt[n] += 1
    span = int(rows[-1]["End_Timestamp"]) - int(rows[0]["Start_Timestamp"])
    ktime = sum(tot.values())
    print(f"{passes} eager batch passes of R = {R} rows: {len(rows)} launches = {len(rows) / passes:.1f} per pass; kernel time "
          f"{ktime / passes / 1e3:.0f} us per pass, first start to last end {span / passes / 1e3:.0f} us per pass\n")
    print("| kernel | launches / pass | us / pass | us / launch | share |")
    print("|---|---|---|---|---|")
    for n, t in tot.most_common():
        print(f"| {n} | {cnt[n] / passes:.1f} | {t / passes / 1e3:.1f} | {t / cnt[n] / 1e3:.1f} | {100.0 * t / ktime:.1f} % |")


if __name__ == "__main__":
    main()
