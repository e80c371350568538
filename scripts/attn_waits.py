"""The per-head decode attention's product kernel (k_attn_head_hd<256, false>, csrc/ops.hip; the body is
attn_head_dev, csrc/attn_impl.h) as the compiler built it, read from the gfx950 assembly:

  * size: code bytes, instructions, conditional branches, `s_waitcnt vmcnt(0)`, v_fma_mix, VGPRs, scratch;
  * the K / V streams: the kernel's text is cut at its s_barrier instructions (front | KQ | softmax | softmax |
    KQV ...), and in the KQ and the KQV part every maximal run of 16-byte global loads with no vmcnt wait
    between them is listed with its length.  A K pass is one run of 8 (the first pass: the prefetch's KPF in the
    front and one run of 8 - KPF), the V steps past the prefetch one run of 8 - VPF behind the passes, a V group
    one run of 8.  A run of one load would be a step with a memory round trip of its own;
  * the front: vmcnt waits between the first vector load and the first s_barrier, v_rcp_iflag_f32 (an integer
    division) anywhere in the kernel, and scripts/kernarg_front.py's figures for the kernel.

    python scripts/attn_waits.py [csrc/ops.hip | file.s] [--json] [-DNAME=VALUE ...]

Compiles the way scripts/kernarg_front.py does.  The cut at the barriers relies on the compiler keeping the
phases in text order; a kernel laid out otherwise shows up as runs in the wrong part, and tests/test_attn_waits.py
fails on it."""
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernarg_front  # noqa: E402  (the compile flags, the demangler)
import rr_waits  # noqa: E402  (the assembly reader)

PRODUCT = "k_attn_head_hd<256, false>("
TAPPED = "k_attn_head_hd<256, true>("
HEADER = os.path.join(kernarg_front.PKG, "csrc", "attn_impl.h")
LOAD16 = re.compile(r"^global_load_dwordx4\b")
VLOAD = re.compile(r"^(global_load|buffer_load|flat_load|scratch_load)")
VMWAIT = re.compile(r"^s_waitcnt\b.*vmcnt\((\d+)\)")


def depths(flags=()):
    """(KPF, VPF): the prefetch depths the header builds with, -DGHIP_AH_* flags applied"""
    d = dict(re.findall(r"^#define (GHIP_AH_\w+) (\w+)", open(HEADER).read(), re.M))
    for f in flags:
        m = re.match(r"-D(GHIP_AH_\w+)=(\w+)", f)
        if m:
            d[m.group(1)] = m.group(2)

    def val(k):
        v = d[k]
        return int(v) if v.isdigit() else val(v)
    return val("GHIP_AH_KPF"), val("GHIP_AH_VPF")


def assembly(path, flags=()):
    """the assembly text of a HIP source (compiled with the product flags) or of a .s file"""
    if path.endswith(".s"):
        return open(path).read()
    r = subprocess.run([kernarg_front.HIPCC, *kernarg_front.FLAGS, *flags, path], cwd=kernarg_front.PKG, capture_output=True,
                       text=True)
    if r.returncode:
        raise RuntimeError(r.stderr[-2000:])
    return r.stdout


def descriptors(text):
    """{demangled kernel: {"vgprs", "code_bytes"}} from the kernel descriptors and the compiler's comments"""
    syms = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    names = kernarg_front.demangle(syms)
    out = {}
    for s in syms:
        body = text[text.index(".amdhsa_kernel " + s):]
        vg = re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", body)
        cl = re.search(r";\s*codeLenInByte\s*=\s*(\d+)", body)
        out[names[s]] = {"vgprs": int(vg.group(1)), "code_bytes": int(cl.group(1)) if cl else None}
    return out


def runs(ins):
    """[(length, index of the first load)] of the maximal runs of 16-byte global loads with no vmcnt wait between"""
    out, n, at = [], 0, None
    for i, t in enumerate(ins):
        if LOAD16.match(t):
            if n == 0:
                at = i
            n += 1
        elif VMWAIT.match(t) and n:
            out.append((n, at))
            n = 0
    if n:
        out.append((n, at))
    return out


def analyse(ins):
    """the figures of one kernel from its instruction list (labels kept as 'LABEL:' lines)"""
    real = [t for t in ins if not t.endswith(":")]
    bars = [i for i, t in enumerate(real) if t.startswith("s_barrier")]
    loads = [i for i, t in enumerate(real) if VLOAD.match(t)]
    out = {"instructions": len(real),
           "cond_branches": sum(t.startswith("s_cbranch") for t in real),
           "vmcnt0": sum(m.group(1) == "0" for m in map(VMWAIT.match, real) if m),
           "fma_mix": sum(t.startswith("v_fma_mix") for t in real),
           "rcp_iflag": sum(t.startswith("v_rcp_iflag_f32") for t in real),
           "barriers": len(bars)}
    if len(bars) < 4 or not loads:
        return out
    out["front_waits"] = [int(VMWAIT.match(t).group(1)) for t in real[loads[0]:bars[0]] if VMWAIT.match(t)]
    out["front_runs"] = [n for n, _ in runs(real[loads[0]:bars[0]])]
    out["kq_runs"] = [n for n, _ in runs(real[bars[0]:bars[1]])]
    out["softmax_loads"] = sum(bool(VLOAD.match(t)) for t in real[bars[1]:bars[3]])
    out["kqv_runs"] = [n for n, _ in runs(real[bars[3]:bars[4] if len(bars) > 4 else len(real)])]
    return out


def run(path="csrc/ops.hip", flags=()):
    """{kernel: figures} of the two head_dim-256 kernels and of k_attn_head (the run-time form)"""
    text = assembly(path, flags)
    with tempfile.NamedTemporaryFile("w", suffix=".s") as f:
        f.write(text)
        f.flush()
        code, scratch = rr_waits.kernels(f.name)
    desc = descriptors(text)
    res = {}
    for name, ins in code.items():
        if name.startswith(PRODUCT) or name.startswith(TAPPED) or name.startswith("k_attn_head("):
            a = analyse(ins)
            a.update(desc[name], scratch=scratch.get(name))
            res[name] = a
    return res


def listing(res):
    rows = []
    for k, a in sorted(res.items()):
        rows.append(k[:60])
        rows.append(f"    {a['code_bytes']} B of code, {a['instructions']} instructions, {a['cond_branches']} conditional branches, "
                    f"{a['vmcnt0']} vmcnt(0), {a['fma_mix']} v_fma_mix, {a['vgprs']} VGPRs, scratch {a['scratch']} B, "
                    f"{a['rcp_iflag']} v_rcp_iflag_f32")
        if "kq_runs" in a:
            rows.append(f"    front: 16-byte load runs {a['front_runs']}, vmcnt waits before the first barrier {a['front_waits']}")
            rows.append(f"    KQ: load runs {a['kq_runs']}   softmax: {a['softmax_loads']} vector loads   KQV: load runs {a['kqv_runs']}")
    return "\n".join(rows)


if __name__ == "__main__":
    srcs = [a for a in sys.argv[1:] if not a.startswith("-")] or ["csrc/ops.hip"]
    flags = [a for a in sys.argv[1:] if a.startswith("-D")]
    res = run(srcs[0], flags)
    print(json.dumps(res, indent=1) if "--json" in sys.argv else listing(res))
