"""The weight ring of the round-pipelined matvecs (csrc/matvec_rr.hip) as the compiler built it:
for every k_matvec_rr kernel of the decode plans (qkv, attn-out and down of Gemma-2B in Q4_0 and Q8_0 under
the engine's default plan and under the bench's tuned one, and the Gemma-7B down), read from the gfx950 assembly

  * the loader path's vmcnt waits, round by round (a ring of D rounds x 2 loads per loader wave: a round
    that is followed by a refill should wait with vmcnt(2(D-1)+1), vmcnt(2(D-1)); the last D rounds count
    down to 0),
  * the waits between the first ring load and the end of the front — the last load of the first issue, or
    the image's last LDS store where the whole ring is issued before the image (with E rounds issued before
    the image is built these waits must stay counted, >= 2E),
  * the number of s_barrier on the loader path and on the carrier path (a mismatch hangs the workgroup),
  * whether the first ring load precedes the first LDS store of the image,
  * the kernel's scratch (.amdhsa_private_segment_fixed_size).

    python scripts/rr_waits.py [csrc/matvec_rr.hip | file.s] [--all] [--json] [-DNAME=VALUE ...]

Compiles the way scripts/kernarg_front.py does.  A path is a walk through the kernel's basic blocks from its
entry.  The walk's rules were written against the block layout of ROCm 7's clang for gfx950 (the comments in
walk() say which layout each rule answers); a walk that goes wrong does not pass quietly: it loses barriers
(the counts differ, or fewer than NR + 1) or finds no rounds, and tests/test_rr_waits.py fails on both.
--all lists every k_matvec_rr of the file.  (kquant.hip's k_matvec_kq_rr has the same loader / carrier shape, but
its weight loads carry no non-temporal flag, so it has no loader marker to walk by: its loads, waits and barriers
are listed by hand in profiles/rr_front/waits_kquant_rr.txt.)"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernarg_front  # noqa: E402  (the compile flags, the demangler)

import subprocess  # noqa: E402

# the kernels the listing is about: k_matvec_rr<WT, PRO, EPI, NR, ...> (Q4_0 = 2, Q8_0 = 8; PRO_NORM = 1,
# PRO_IMG = 4; EPI_STORE = 0, EPI_ADD = 1)
PLAN = {  # "image" = the activation comes as the Q8_0 image (PRO_IMG), "f32" = as floats (PRO_F32)
    "qkv q4_0": r"^k_matvec_rr<2, 1, 0, 1,",
    "qkv q8_0": r"^k_matvec_rr<8, 1, 0, 2,",
    "attn-out q4_0 image": r"^k_matvec_rr<2, 4, 1, 1,",  # the engine's default plan
    "attn-out q4_0 f32": r"^k_matvec_rr<2, 0, 1, 1,",    # the bench's tuned plan
    "attn-out q8_0 image": r"^k_matvec_rr<8, 4, 1, 2,",
    "attn-out q8_0 f32": r"^k_matvec_rr<8, 0, 1, 2,",
    "down q4_0 image": r"^k_matvec_rr<2, 4, 1, 8,",      # the bench's tuned plan
    "down q4_0 f32": r"^k_matvec_rr<2, 0, 1, 8,",        # the engine's default plan
    "down q8_0 image": r"^k_matvec_rr<8, 4, 1, 16,",
    "down q8_0 f32": r"^k_matvec_rr<8, 0, 1, 16,",
    "down 7B q4_0 image": r"^k_matvec_rr<2, 4, 1, 12,",
    "down 7B q4_0 f32": r"^k_matvec_rr<2, 0, 1, 12,",
}
BRANCH = re.compile(r"^(s_branch|s_cbranch_\w+)\s+(\S+)")
RING_LOAD = re.compile(r"^global_load_\w+\b.*\bnt\b")
VMCNT = re.compile(r"^s_waitcnt\b.*vmcnt\((\d+)\)")


def kernels(path, extra_flags=()):
    """({demangled kernel name: [instruction text, ...] with labels kept as 'LABEL:' lines},
    {demangled kernel name: scratch bytes per lane})"""
    if path.endswith(".s"):  # assembly made earlier (another checkout's, say)
        lines = open(path).read().splitlines()
    else:
        r = subprocess.run([kernarg_front.HIPCC, *kernarg_front.FLAGS, *extra_flags, path], cwd=kernarg_front.PKG,
                           capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError(r.stderr[-2000:])
        lines = r.stdout.splitlines()
    syms = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m]
    names = kernarg_front.demangle(syms)
    out, cur, scratch, desc = {}, None, {}, None
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            desc = m.group(1)
        m = re.match(r"\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", ln)
        if m and desc:
            scratch[names[desc]] = int(m.group(1))
        m = re.match(r"^(\w+):", ln)
        if m and m.group(1) in names:
            cur = out.setdefault(names[m.group(1)], [])
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        t = ln.split(";")[0].strip()
        if t and (not t.startswith(".") or re.match(r"^\.LBB\w+:", t)):
            cur.append(t)
    return out, scratch


class Block:
    def __init__(self, label):
        self.label, self.ins, self.succ, self.fall, self.target = label, [], [], None, None


def blocks_of(ins):
    """basic blocks in text order; succ = [fall-through, branch target] as block indices"""
    blocks, cur = [], Block(None)
    for t in ins:
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            if cur.ins or cur.label:
                blocks.append(cur)
            cur = Block(m.group(1))
            continue
        cur.ins.append(t)
        if BRANCH.match(t) or t.startswith("s_endpgm"):
            blocks.append(cur)
            cur = Block(None)
    if cur.ins or cur.label:
        blocks.append(cur)
    by_label = {b.label: i for i, b in enumerate(blocks) if b.label}
    for i, b in enumerate(blocks):
        last = b.ins[-1] if b.ins else ""
        m = BRANCH.match(last)
        if last.startswith("s_endpgm"):
            continue
        if m:
            b.target = by_label.get(m.group(2))
            if m.group(1) != "s_branch" and i + 1 < len(blocks):
                b.fall = i + 1
        elif i + 1 < len(blocks):
            b.fall = i + 1
        b.succ = [s for s in (b.fall, b.target) if s is not None]
    return blocks


def _count(b, pat):
    return sum(1 for t in b.ins if re.match(pat, t))


def _region(blocks, start, stop):
    """the blocks reached from start without passing stop"""
    seen, todo = {start}, [start]
    while todo:
        for s in blocks[todo.pop()].succ:
            if s != stop and s not in seen:
                seen.add(s)
                todo.append(s)
    return seen


def walk(blocks, for_loader):
    """block indices of one wave kind's way through the kernel, from the entry.

    Markers: a loader issues the weight loads (the only non-temporal loads of these kernels), the carrier raises
    its priority (s_setprio).  At a two-way branch the walk falls through, because that is where the compiler puts
    what runs: loop exits, lane-masked skips (s_cbranch_execz) and the norm check's out-of-line fallback are the
    branch targets.  The rules below are the exceptions, each with the layout it was written against."""
    def ring(b):
        return any(RING_LOAD.match(t) for t in b.ins)

    def prio(b):
        return any(t.startswith("s_setprio") for t in b.ins)

    def chain(b):  # a carrier's round: the fma chain over a stash slot
        return _count(b, r"v_fma(c)?_f32") >= 32 and not _count(b, r"v_dot4")

    def stash(b):  # a loader's round: dot products into the stash slot
        return _count(b, r"v_dot4") and _count(b, r"ds_write")

    mine, other, avoid = (ring, prio, chain) if for_loader else (prio, ring, stash)
    order, seen, i = [], set(), 0
    while i is not None and i not in seen:
        seen.add(i)
        order.append(i)
        cand = [s for s in blocks[i].succ if s not in seen]
        if len(cand) == 2:
            fall, target = cand
            if blocks[i].ins[-1].startswith("s_cbranch_execnz"):
                # layout: `s_cbranch_execnz BODY` ("any lane left") with the skip falling through — the image
                # builder's `if (item < T)` ladder of the R 2 kernels.  Read as body = target.
                cand = [target, fall]
                fall, target = cand
            rf, rt = _region(blocks, fall, target), _region(blocks, target, fall)
            mf, mt = (any(mine(blocks[k]) for k in r) for r in (rf, rt))
            of, ot = (any(other(blocks[k]) for k in r) for r in (rf, rt))
            if avoid(blocks[fall]) and not avoid(blocks[target]):
                # layout (joined form): per round `s_cbranch_vccnz STASH` with the carrier's chain falling
                # through.  A chain is >= 32 v_fma and no v_dot4, a stash is v_dot4 and LDS stores.
                cand = [target]
            elif target in _region(blocks, fall, None):
                # layout (split form): `s_cbranch_scc0 L; <carrier's whole path>; L: s_cbranch_vccz END;
                # <loader's whole path>` — the two paths one behind the other, each under its guard (the
                # structurizer's form; the guard after the carrier's path is never taken at run time).  A
                # guarded region that holds the other kind's marker and not this kind's is skipped.
                # layout: `s_cbranch_execz AFTER; <preheader>; LOOP: ...; s_cbranch_execnz LOOP; AFTER:` — a
                # guarded loop is skipped too: here the image builder's iterations past the prefetched
                # registers and the zeroing of padded blocks, neither of which runs at a supported shape.
                k = fall  # (straight into the loop: a guard around more than the loop is walked into)
                while len(blocks[k].succ) == 1 and k not in _region(blocks, blocks[k].succ[0], target):
                    k = blocks[k].succ[0]
                loop = any(k in _region(blocks, s, target) for s in blocks[k].succ)
                if (of or loop) and not mf:
                    cand = [target]
            elif fall not in _region(blocks, target, None):
                # layout (split form, Q8_0 kernels): `s_cbranch_scc1 CARRIER; s_cbranch_vccnz LOADER; END:
                # s_endpgm; CARRIER: ...; s_branch END; LOADER: ...` — two ways that do not meet again: the
                # one with this kind's marker, or without the other's
                if (mt and not mf) or (mt == mf and of and not ot):
                    cand = [target]
        i = cand[0] if cand else None
    return order


def analyse(name, ins):
    """the figures of one kernel, or None if it has no loader / carrier split"""
    blocks = blocks_of(ins)
    if not any(RING_LOAD.match(t) for b in blocks for t in b.ins) or not any(t.startswith("s_setprio") for b in blocks for t in b.ins):
        return None
    lwalk, cwalk = walk(blocks, True), walk(blocks, False)
    ev = []  # the loader's way: ("load" | "wait" | "barrier" | "store", value)
    for i in lwalk:
        for t in blocks[i].ins:
            m = VMCNT.match(t)
            if RING_LOAD.match(t):
                ev.append(("load", 0))
            elif m:
                ev.append(("wait", int(m.group(1))))
            elif t.startswith("s_barrier"):
                ev.append(("barrier", 0))
            elif t.startswith("ds_write"):
                ev.append(("store", 0))
    carrier_barriers = sum(_count(blocks[i], r"s_barrier") for i in cwalk)
    shared = [i for i in set(lwalk) & set(cwalk) if _count(blocks[i], r"s_barrier")]
    targs = [int(v) for v in re.findall(r"-?\d+", name[name.index("<"):])] if "<" in name else []
    bars = [k for k, e in enumerate(ev) if e[0] == "barrier"]
    loads = [k for k, e in enumerate(ev) if e[0] == "load"]
    stores = [k for k, e in enumerate(ev) if e[0] == "store"]
    out = {"barriers": {"loader": len(bars), "carrier": carrier_barriers},
           "split": not shared,  # no barrier that both kinds of wave reach in the same block
           "ring_first": bool(loads and stores and loads[0] < stores[0])}
    shape = None  # (NR, D, E) from the template arguments
    if len(targs) >= 6 and name.startswith("k_matvec_rr<"):
        shape = (targs[3], min(targs[5], targs[3]), min(targs[6], targs[5], targs[3]) if len(targs) > 6 else 0)
    if shape and len(bars) >= shape[0] + 1:
        nr, d, e = shape
        end = bars[-nr:]      # the barrier that ends round r
        pre = bars[-nr - 1]   # the barrier in front of the rounds: the first issue is complete before it
        first_issue = [k for k in loads if k < pre]
        # the front ends with the last load of the first issue, or (E = D: all of it in front of the image)
        # with the image's last store
        front_end = first_issue[-1] if e < d else max([k for k in stores if k < pre] + [first_issue[-1]])
        rounds = []
        for r in range(nr):
            lo = front_end if r == 0 else end[r - 1]
            if r > 0:  # behind round r-1's refill, wherever the scheduler put the next round's wait
                refill = [k for k in loads if (end[r - 2] if r > 1 else pre) < k < end[r - 1]]
                lo = refill[-1] if refill else lo
            nxt = [k for k in loads if lo < k < end[r]]
            hi = nxt[0] if nxt else end[r]
            rounds.append([v for k, (what, v) in enumerate(ev) if what == "wait" and lo < k < hi])
        out.update(nr=nr, d=d, e=e, rounds=rounds, lpr=len(first_issue) // d,  # lpr: loads per round and wave
                   front=[v for k, (what, v) in enumerate(ev) if what == "wait" and first_issue[0] < k < front_end])
    return out


def steady(a):
    """the rule tests/test_rr_waits.py holds: [] or the list of complaints about a k_matvec_rr's waits"""
    bad = []
    nr, d, lpr = a["nr"], a["d"], a["lpr"]
    for r, w in enumerate(a["rounds"]):
        want = lpr * ((d - 1) if r + d < nr else (nr - 1 - r))  # loads of later rounds still in flight
        if not w or w[-1] != want or min(w) < want:  # (a higher count in front is a weaker wait: harmless)
            bad.append(f"round {r}: waits {w}, want down to vmcnt({want})")
    return bad


def listing(res):
    rows = []
    for k, a in res.items():
        rows.append(k[:110])
        if "rounds" in a:
            rows.append(f"    NR {a['nr']}  D {a['d']}  E {a['e']}  {a['lpr']} loads per round   loader waits per round: "
                        + " ".join("(" + ",".join(map(str, w)) + ")" for w in a["rounds"]))
            rows.append(f"    waits inside the front: {a['front'] if a['front'] else '-'}")
            if a["nr"] > a["d"]:
                rows.append("    steady state: " + ("yes" if not steady(a) else "NO — " + "; ".join(steady(a))))
            else:
                rows.append("    one-shot ring (no refill): joined form")
        rows.append(f"    s_barrier: loader path {a['barriers']['loader']}, carrier path {a['barriers']['carrier']}"
                    f"   paths split: {'yes' if a['split'] else 'no (they rejoin)'}"
                    f"   first ring load before the first LDS store: {'yes' if a['ring_first'] else 'no'}"
                    f"   scratch: {a.get('scratch')} B")
    return "\n".join(rows)


def run(path="csrc/matvec_rr.hip", extra_flags=(), show_all=False):
    res = {}
    code, scratch = kernels(path, extra_flags)
    for name, ins in sorted(code.items()):
        if name.startswith("k_matvec_rr<") and (show_all or any(re.match(p, name) for p in PLAN.values())):
            a = analyse(name, ins)
            if a:
                a["scratch"] = scratch.get(name)
                res[name] = a
    return res


if __name__ == "__main__":
    srcs = [a for a in sys.argv[1:] if not a.startswith("-")] or ["csrc/matvec_rr.hip"]
    flags = [a for a in sys.argv[1:] if a.startswith("-D")]
    res = {}
    for src in srcs:
        res.update(run(src, flags, "--all" in sys.argv))
    print(json.dumps(res, indent=1) if "--json" in sys.argv else listing(res))
