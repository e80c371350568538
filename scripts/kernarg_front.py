"""The launch front of the decode kernels: for every kernel of a HIP source that the
benched decode graph runs, the kernarg preload length (dwords of leading scalar parameters the command
processor puts into user SGPRs) and the kernarg s_loads, if any, that are waited for before the
kernel's first vector memory load, after the preload entry point.

    python scripts/kernarg_front.py csrc/matvec_rr.hip csrc/ops.hip [--all] [--json]

Compiles to assembly with the product flags (the way scripts/reg_usage.py compiles).  The scan is in
text order from the entry to the first vector load: a kernarg load is an s_load whose base is the
kernarg segment pointer s[0:1] (these kernels enable no other pointer SGPRs, which is checked), and it
counts as waited for when an s_waitcnt with lgkmcnt(0) follows it before that first vector load."""
import json
import os
import re
import subprocess
import sys

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gemma.ggml_amd")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mllvm", "-amdgpu-mfma-vgpr-form=1",
         "-mllvm", "-amdgpu-kernarg-preload-count=16", "-I../include", "-Icsrc", "-S", "--cuda-device-only", "-o", "-"]
# kernels of the benched decode graph (demangled names, namespaces stripped)
DECODE = re.compile(r"^(k_matvec_rr<|k_matvec<|k_attn_head\(|k_advance\()")
VLOAD = re.compile(r"^(global_load|buffer_load|flat_load|scratch_load)")


def demangle(names):
    tool = "/opt/rocm/llvm/bin/llvm-cxxfilt"
    r = subprocess.run([tool if os.path.exists(tool) else "c++filt"], input="\n".join(names), capture_output=True, text=True,
                       check=True)
    out = {}
    for n, d in zip(names, r.stdout.splitlines()):
        d = re.sub(r"^void ", "", d).replace("ghip::(anonymous namespace)::", "").replace("ghip::", "")
        out[n] = d
    return out


def fronts(path, extra_flags=()):
    """{demangled kernel: {"preload": dwords, "waited": ["s_load_... offset", ...], "first_vload": text}}"""
    r = subprocess.run([HIPCC, *FLAGS, *extra_flags, path], cwd=PKG, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(r.stderr[-2000:])
    lines = r.stdout.splitlines()
    # kernel descriptors: preload length and which pointer SGPRs are enabled
    desc, cur = {}, None
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            cur = m.group(1)
            desc[cur] = {}
            continue
        m = re.match(r"\s*\.amdhsa_(\w+)\s+(\d+)", ln)
        if m and cur:
            desc[cur][m.group(1)] = int(m.group(2))
        if ".end_amdhsa_kernel" in ln:
            cur = None
    names = demangle(list(desc))
    start = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\w+):", ln)
        if m and m.group(1) in desc:
            start[m.group(1)] = i
    out = {}
    for sym, i0 in start.items():
        d = desc[sym]
        preload = d.get("user_sgpr_kernarg_preload_length", 0)
        others = [k for k in ("user_sgpr_dispatch_ptr", "user_sgpr_queue_ptr", "user_sgpr_private_segment_buffer",
                              "user_sgpr_dispatch_id", "user_sgpr_flat_scratch_init") if d.get(k, 0)]
        i = i0 + 1
        if preload:  # skip the compatibility entry (s_load of the preloaded dwords for firmware without the feature)
            while i < len(lines) and ".p2align" not in lines[i]:
                i += 1
        pending, waited, first = [], [], None
        for ln in lines[i:]:
            t = ln.strip()
            if t.startswith(".Lfunc_end"):  # (an s_endpgm may come first: an early exit in front of the body)
                break
            if VLOAD.match(t):
                first = t
                break
            m = re.match(r"(s_load_\w+)\s+\S+,\s*(s\[\d+:\d+\]),\s*(\S+)", t)
            if m and (m.group(2) == "s[0:1]" or others):
                pending.append(f"{m.group(1)} {m.group(3)}")
            if t.startswith("s_waitcnt") and "lgkmcnt(0)" in t and pending:
                waited += pending
                pending = []
        out[names[sym]] = {"preload": preload, "waited": waited, "first_vload": first}
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    show_all, as_json = "--all" in sys.argv, "--json" in sys.argv
    res = {}
    for src in args:
        for k, v in fronts(src).items():
            if show_all or DECODE.match(k):
                res[k] = v
    if as_json:
        print(json.dumps(res, indent=1))
    else:
        for k, v in sorted(res.items()):
            w = ", ".join(v["waited"]) if v["waited"] else "-"
            print(f"{k[:100]:100s} preload {v['preload']:2d}  waited before the first vector load: {w}")
