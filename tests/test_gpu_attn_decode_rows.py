"""GPU: the decode attention's launch forms, each alone (gemma_test_attn_decode_rows), bit for bit against
orc_attn_decode_row on the single-row inputs of tests/attn_adversary.py (decode_case).

form 0  k_attn_head, 1 / 2 / 4 / 8 workgroups per head (dsplit)
form 1  k_attn_decode, the position-split form with its in-kernel hand-off
form 2  k_attn_slots: R rows, each on its own slot's caches at its own position, one launch
form 3  k_rows_rope_kv + k_attn_slot_rows: several rows per slot, every K / V operand read from the cache

Every comparison is bit equality: out; the scores on j <= pos and -inf on pos < j < n_kv; P16 on j < n_kv; K row
pos and V column pos; every other cache word unchanged; where requested the Q8_0 image of out (O.image_of) and
its Q8_K image (O.quantize_q8_K), and no word of a buffer outside what the form owns.  The score comparison is
what pins the KQ accumulation: on N(0,1) inputs a wrong quad fold changes half of the score words and (almost)
no output word; cancel_kq rows make a wrong step order visible in the outputs too
(tests/test_attn_decode_adversary.py has the measured shares).

The inputs put finite non-zero garbage into the cache at the row's own position (a kernel that reads its own K
row or V column from the cache instead of the row is wrong) and, for `stale`, past it (a rewind's leftovers).
With the identity RoPE row (cos 1, sin 0) and q_scale 1 the kernel's q16 / k16 are the case's f16 words; `normal`
rows are N(0,1) under the real RoPE row and 1 / sqrtf(hd); `zero_v` has one kv head's V dims 32..63 zero (an
image block with d == 0).  underflow rows with 8 heads carry two tied maxima (attn_adversary.underflow_kind)."""
import ctypes as C
import functools

import numpy as np
import pytest

import attn_adversary as A
import oracle_ctypes as O

gpu = pytest.mark.gpu
U32 = np.uint32
OUT_S, W_S, P_S, ACT_S, DA_S, Q8K_S = np.float32(-7.5), np.float32(123.25), 0xDEAD, 0xA5A5A5A5, np.float32(-3.0), 0x5A
NEG_INF = 0xFF800000
CASES = A.CASES + ("zero_v", "normal")
HEADS = [(2, 1), (4, 2), (8, 1), (2, 2)]
POS0 = [0, 1, 7, 8, 30, 31, 32, 33, 63, 64, 255, 256, 257, 287]


class AttnRowsArgs(C.Structure):
    """struct gemma_test_attn_rows_args (include/gemma_hpc.h)"""
    _fields_ = [(n, C.c_int) for n in ("form", "R", "n_slots", "H", "Hkv", "hd", "ctx", "dsplit", "nwg", "rope_identity")] + \
               [("rope_base", C.c_float), ("q_scale", C.c_float), ("qkv", C.c_void_p), ("ldqkv", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("pos", "slot", "kc", "vc", "out", "dbg_w", "dbg_p", "img_act", "img_da", "img_q8k",
                                          "sync_out")] + [("err_out", C.c_int)]


def _lib():
    import gemma_hip as G
    L = G.lib()
    L.gemma_test_attn_decode_rows.restype = C.c_int
    L.gemma_test_attn_decode_rows.argtypes = [C.POINTER(AttnRowsArgs)]
    return G, L


def _positions(ctx):
    return sorted({p for p in POS0 + [ctx - 2, ctx - 1] if 0 <= p < ctx})


def _q_scale(hd):
    return float(np.float32(1.0) / np.sqrt(np.float32(hd)))


@functools.lru_cache(maxsize=512)
def _qkv_row(name, i, H, Hkv, hd):
    """a q | k | v row of the case's family, cheap: decode_case at a small position (the patterns of a case do
    not depend on the position); for rows that follow a slot's first row"""
    return _row(name, 1 + i % 8, H, Hkv, hd, 32)[0]


def _row(name, pos, H, Hkv, hd, ctx):
    """-> (qkv, kc [ctx][kvw], vc [kvw][ctx], identity?) of one row"""
    if name == "normal":
        rng = np.random.default_rng([5, pos, H, Hkv, hd])
        kvw = Hkv * hd
        qkv = (rng.standard_normal((H + 2 * Hkv) * hd) * 2.0).astype(np.float32)
        kc, vc = np.zeros((ctx, kvw), np.uint16), np.zeros((kvw, ctx), np.uint16)
        kc[:pos] = rng.standard_normal((pos, kvw)).astype(np.float16).view(np.uint16)
        vc[:, :pos] = rng.standard_normal((kvw, pos)).astype(np.float16).view(np.uint16)
        kc[pos], vc[:, pos] = A._garbage(rng, kvw), A._garbage(rng, kvw)
        return qkv, kc, vc, False
    if name == "zero_v":
        cs = A.decode_case("benign", pos, H, Hkv, hd, ctx, zero_v=(Hkv - 1, 32, 32))
    else:
        cs = A.decode_case(name, pos, H, Hkv, hd, ctx)
    return cs["qkv"], cs["kc"], cs["vc"], True


def _rope_row(pos, hd, identity):
    return A.identity_rope(hd) if identity else np.concatenate(A.rope_tables(pos, hd))


class Batch:
    """rows (qkv, pos, slot) over n_slots cache pairs, all identity-RoPE or all real; the oracle's results"""

    def __init__(self, H, Hkv, hd, ctx, identity):
        self.H, self.Hkv, self.hd, self.ctx, self.identity = H, Hkv, hd, ctx, identity
        self.qkv, self.pos, self.slot, self.kc, self.vc, self.tag = [], [], [], [], [], []

    def add_slot(self, kc, vc):
        self.kc.append(kc)
        self.vc.append(vc)
        return len(self.kc) - 1

    def add_row(self, qkv, pos, slot, tag):
        self.qkv.append(qkv)
        self.pos.append(pos)
        self.slot.append(slot)
        self.tag.append(tag)

    def add_case(self, name, pos):
        qkv, kc, vc, ident = _row(name, pos, self.H, self.Hkv, self.hd, self.ctx)
        assert ident == self.identity
        self.add_row(qkv, pos, self.add_slot(kc, vc), (name, pos))

    def freeze(self):
        """the inputs as arrays and the oracle applied row by row (rows of a slot in the order given)"""
        H, Hkv, hd, ctx = self.H, self.Hkv, self.hd, self.ctx
        self.kc0, self.vc0 = np.ascontiguousarray(np.stack(self.kc)), np.ascontiguousarray(np.stack(self.vc))
        self.kc = self.vc = None
        self.qkv = np.ascontiguousarray(np.stack(self.qkv)) if self.qkv else np.zeros((1, (H + 2 * Hkv) * hd), np.float32)
        self.kc_ref, self.vc_ref = self.kc0.copy(), self.vc0.copy()
        qs = 1.0 if self.identity else _q_scale(hd)
        self.ref = [O.attn_decode_row(self.qkv[r], self.kc_ref[s], self.vc_ref[s], p, H, Hkv, hd, ctx,
                                      _rope_row(p, hd, self.identity), qs) for r, (p, s) in enumerate(zip(self.pos, self.slot))]
        return self


def _run(b, form, dsplit=1, taps=True, img=False, q8k=False, nwg=0, R=None):
    """one call of the entry on copies of the batch's caches -> dict of what came back"""
    G, L = _lib()
    H, hd, ctx = b.H, b.hd, b.ctx
    R = len(b.pos) if R is None else R
    Rn = max(R, 1)
    nb = (H * hd + 31) // 32
    o = dict(kc=b.kc0.copy(), vc=b.vc0.copy(), out=np.full((Rn, H * hd), OUT_S, np.float32),
             w=np.full((Rn, H, ctx), W_S, np.float32) if taps else None, p=np.full((Rn, H, ctx), P_S, np.uint16) if taps else None,
             act=np.full((Rn, (nb + 3) // 4 * 32), ACT_S, np.uint32) if img else None,
             da=np.full((Rn, nb), DA_S, np.float32) if img else None,
             q8k=np.full((Rn, H * 292), Q8K_S, np.uint8) if q8k else None, sync=np.full(2 * b.Hkv, -1, np.int32))
    pos = np.array(list(b.pos[:R]) + [0] * (Rn - min(R, len(b.pos))), np.int32)
    slot = np.array(list(b.slot[:R]) + [0] * (Rn - min(R, len(b.slot))), np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data
    t = AttnRowsArgs(form=form, R=R, n_slots=len(o["kc"]), H=H, Hkv=b.Hkv, hd=hd, ctx=ctx, dsplit=dsplit, nwg=nwg,
                     rope_identity=int(b.identity), rope_base=10000.0, q_scale=1.0 if b.identity else _q_scale(hd),
                     qkv=b.qkv.ctypes.data, ldqkv=b.qkv.shape[1], pos=pos.ctypes.data, slot=slot.ctypes.data, kc=ptr(o["kc"]),
                     vc=ptr(o["vc"]), out=ptr(o["out"]), dbg_w=ptr(o["w"]), dbg_p=ptr(o["p"]), img_act=ptr(o["act"]),
                     img_da=ptr(o["da"]), img_q8k=ptr(o["q8k"]), sync_out=ptr(o["sync"]), err_out=-1)
    o["r"] = L.gemma_test_attn_decode_rows(C.byref(t))
    o["why"], o["err"] = G.last_error(), t.err_out
    return o


def _check(b, o, what):
    """every assertion of the module on one call's results; -> list of failure lines (empty: all equal)"""
    H, Hkv, hd, ctx = b.H, b.Hkv, b.hd, b.ctx
    if o["r"] != 0:
        return [f"{what}: refused ({o['r']}: {o['why']})"]
    bad = []
    for r, (pos, (ref, w, p)) in enumerate(zip(b.pos, b.ref)):
        n_kv, where = O.attn_n_kv(pos, ctx), f"{what} row {r} {b.tag[r]}"
        got = o["out"][r]
        d = np.flatnonzero(got.view(U32) != ref.view(U32))
        if d.size:
            bad.append(f"{where}: out, {d.size} of {got.size} words; first head {d[0] // hd} dim {d[0] % hd}: "
                       f"{got[d[0]]!r} != {ref[d[0]]!r}; heads {sorted(set((d // hd).tolist()))}")
        if o["w"] is not None:
            gw, gp = o["w"][r], o["p"][r]
            d = np.argwhere(gw[:, :pos + 1].view(U32) != w[:, :pos + 1].view(U32))
            if len(d):
                h, j = d[0]
                bad.append(f"{where}: scores, {len(d)} of {H * (pos + 1)} words; first head {h} key {j}: {gw[h, j]!r} != {w[h, j]!r}")
            if not (gw[:, pos + 1:n_kv].view(U32) == NEG_INF).all():
                bad.append(f"{where}: scores past pos are not -inf")
            if not ((gw[:, n_kv:] == W_S).all() and (gp[:, n_kv:] == P_S).all()):
                bad.append(f"{where}: taps written past n_kv")
            d = np.argwhere(gp[:, :n_kv] != p[:, :n_kv])
            if len(d):
                h, j = d[0]
                bad.append(f"{where}: P16, {len(d)} of {H * n_kv} words; first head {h} key {j}: {gp[h, j]:#06x} != {p[h, j]:#06x}")
        if o["act"] is not None:
            qs, da = O.image_of(ref)
            used = np.zeros(o["act"].shape[1], bool)
            for blk in range(qs.shape[0]):
                idx = O.image_words(blk)
                used[idx] = True
                if not np.array_equal(o["act"][r][idx], qs[blk]) or o["da"][r, blk:blk + 1].view(U32) != da[blk:blk + 1].view(U32):
                    bad.append(f"{where}: Q8_0 image block {blk} (head {blk // (hd // 32)}): scale {o['da'][r, blk]!r} != {da[blk]!r}")
                    break
            if not (o["act"][r][~used] == ACT_S).all():
                bad.append(f"{where}: image words outside out's blocks written")
        if o["q8k"] is not None:
            want = O.quantize_q8_K(ref[None])[0]
            if not np.array_equal(o["q8k"][r], want):
                bad.append(f"{where}: Q8_K image, {int((o['q8k'][r] != want).sum())} of {want.size} bytes")
    for s in range(len(b.kc0)):
        for nm, got, want, was in (("K", o["kc"][s], b.kc_ref[s], b.kc0[s]), ("V", o["vc"][s].T, b.vc_ref[s].T, b.vc0[s].T)):
            rows = np.flatnonzero((got != want).any(axis=1))
            if rows.size:
                own = [p for p, sl in zip(b.pos, b.slot) if sl == s]
                bad.append(f"{what} slot {s} (rows at {own}): {nm} cache differs at positions {rows[:8].tolist()} "
                           f"({'its own rows' if set(rows.tolist()) <= set(own) else 'positions no row of the call owns'})")
    return bad


def _assert_none(fails):
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:8])


# ---- form 0: the per-head kernel -----------------------------------------------------------------------

def _chunks(n_rows, slot_bytes, cap=48 << 20):
    per = max(1, cap // slot_bytes)
    return [range(i, min(i + per, n_rows)) for i in range(0, n_rows, per)]


@gpu
@pytest.mark.parametrize("ctx", [32, 96, 320, 2048])
@pytest.mark.parametrize("hd", [64, 128, 256])
def test_per_head_form(hd, ctx):
    """every case at every position (V-patch lane, dword and half; both KQV paths around n_kv 256; the cap
    n_kv == ctx at ctx - 2 and ctx - 1; ctx < 256: the prefetch's clamps), every dsplit the head_dim takes, two of
    the four head shapes per (head_dim, ctx) (all four per head_dim and per ctx); the Q8_0 image at every dsplit,
    the Q8_K image at head_dim 256"""
    i = [64, 128, 256].index(hd) + [32, 96, 320, 2048].index(ctx)
    fails = []
    for H, Hkv in (HEADS[i % 4], HEADS[(i + 2) % 4]):
        items = [(name, pos) for name in CASES for pos in _positions(ctx)]
        for ident in (True, False):
            sel = [it for it in items if (it[0] != "normal") == ident]
            for ch in _chunks(len(sel), 4 * ctx * Hkv * hd):
                b = Batch(H, Hkv, hd, ctx, ident)
                for k in ch:
                    b.add_case(*sel[k])
                b.freeze()
                for ds in (1, 2, 4, 8):
                    if hd % (32 * ds) == 0:
                        o = _run(b, 0, ds, img=True, q8k=hd == 256 and ds == 1)
                        fails += _check(b, o, f"H {H} Hkv {Hkv} hd {hd} ctx {ctx} dsplit {ds}")
    _assert_none(fails)


@gpu
def test_per_head_form_long_context():
    """ctx 16384 (a 99 KiB LDS image: the launcher's attribute path), Hkv 1, H 2, the last two positions"""
    H, Hkv, hd, ctx = 2, 1, 256, 16384
    b = Batch(H, Hkv, hd, ctx, True)
    for name in ("cancel_kq", "cancel_kqv", "underflow"):
        for pos in (ctx - 2, ctx - 1):
            b.add_case(name, pos)
    b.freeze()
    fails = _check(b, _run(b, 0, 1, img=True, q8k=True), "ctx 16384 dsplit 1") + _check(b, _run(b, 0, 4, img=True), "ctx 16384 dsplit 4")
    _assert_none(fails)


# ---- form 1: the position-split kernel -----------------------------------------------------------------

def _successive(name, start, n, H, Hkv, hd, ctx):
    """n rows at start .. start + n - 1 on one slot: the first from decode_case (its history and garbage), the
    rest rows of the same family; the oracle row by row on the same caches"""
    qkv, kc, vc, ident = _row(name, start, H, Hkv, hd, ctx)
    b = Batch(H, Hkv, hd, ctx, ident)
    s = b.add_slot(kc, vc)
    b.add_row(qkv, start, s, (name, start))
    for i in range(1, n):
        b.add_row(_qkv_row(name, i, H, Hkv, hd), start + i, s, (name, start + i))
    return b.freeze()


SPLIT_STARTS = {96: [0, 29, 92], 512: [254, 508], 4096: [254, 2045, 4092]}


@gpu
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2), (8, 1)], ids=["G1", "G2", "G8"])
@pytest.mark.parametrize("hd", [64, 256, 512])
def test_split_form(hd, H, Hkv):
    """four successive positions per case on ONE scratch allocation (positions 255 .. 257, 2047 / 2048, 4095 and
    ctx - 1 among them; ctx 96 below the staged V width; G 8 at ctx 4096 past 64 KiB of LDS): every launch after
    the first runs on the counters the one before left, which must be zero at the end, the error word 0; the
    Q8_0 image's blocks are indexed by workgroup"""
    fails = []
    for ctx, starts in SPLIT_STARTS.items():
        for start in starts:
            for name in A.CASES + ("normal",):
                b = _successive(name, start, 4, H, Hkv, hd, ctx)
                o = _run(b, 1, img=True)
                what = f"split H {H} Hkv {Hkv} hd {hd} ctx {ctx} from {start} {name}"
                fails += _check(b, o, what)
                if o["r"] == 0 and (o["sync"].any() or o["err"] != 0):
                    fails.append(f"{what}: counters {o['sync'].tolist()} error word {o['err']} after the last launch")
    _assert_none(fails)


# ---- form 2: one row per slot --------------------------------------------------------------------------

SLOT_SHAPES = [(4, 2, 256), (8, 1, 128), (2, 1, 64)]


@gpu
@pytest.mark.parametrize("dsplit", [1, 2])
@pytest.mark.parametrize("H,Hkv,hd", SLOT_SHAPES)
def test_slots_form(H, Hkv, hd, dsplit):
    """R = 9 rows on 9 slots at their own positions in one launch (the placement's & 7 wraps), per case; one row
    alone with the taps (they are indexed by head only)"""
    ctx = 320
    fails = []
    for name in A.CASES + ("normal",):
        b = Batch(H, Hkv, hd, ctx, name != "normal")
        for pos in (0, 31, 32, 63, 255, 256, 300, ctx - 2, ctx - 1):
            b.add_case(name, pos)
        b.freeze()
        fails += _check(b, _run(b, 2, dsplit, taps=False), f"slots H {H} hd {hd} dsplit {dsplit} {name} R 9")
        for pos in (31, 300):
            b = Batch(H, Hkv, hd, ctx, name != "normal")
            b.add_case(name, pos)
            b.freeze()
            fails += _check(b, _run(b, 2, dsplit), f"slots H {H} hd {hd} dsplit {dsplit} {name} R 1")
    _assert_none(fails)


@gpu
@pytest.mark.parametrize("dsplit", [1, 2])
def test_slots_form_64_rows(dsplit):
    """the widest pass: 64 slots at positions 0 .. 63 of ctx 64, the cases by turns"""
    b = Batch(2, 1, 64, 64, True)
    for pos in range(64):
        b.add_case(A.CASES[pos % len(A.CASES)], pos)
    b.freeze()
    _assert_none(_check(b, _run(b, 2, dsplit, taps=False), f"slots R 64 dsplit {dsplit}"))


# ---- form 3: several rows per slot ---------------------------------------------------------------------

def _slot_rows_batch(name, H, Hkv, hd, ctx, spans):
    """spans [(first position, rows)]: one slot each, `stale` garbage past the slot's first position (so past
    its last row too; the rows between overwrite theirs), the base case `name`"""
    ident = name != "normal"
    b = Batch(H, Hkv, hd, ctx, ident)
    for first, m in spans:
        if ident:
            cs = A.decode_case("stale", first, H, Hkv, hd, ctx, base=name)
            qkv, kc, vc = cs["qkv"], cs["kc"], cs["vc"]
        else:
            qkv, kc, vc, _ = _row(name, first, H, Hkv, hd, ctx)
            rng = np.random.default_rng([9, first])
            kc[first + 1:] = A._garbage(rng, kc[first + 1:].shape)
            vc[:, first + 1:] = A._garbage(rng, vc[:, first + 1:].shape)
        s = b.add_slot(kc, vc)
        b.add_row(qkv, first, s, (name, first))
        for i in range(1, m):
            b.add_row(_qkv_row(name, i, H, Hkv, hd), first + i, s, (name, first + i))
    return b.freeze()


@gpu
@pytest.mark.parametrize("dsplit", [1, 2])
@pytest.mark.parametrize("H,Hkv,hd", SLOT_SHAPES)
def test_slot_rows_form(H, Hkv, hd, dsplit):
    """T = 15: slot A 5 rows from 29 (n_kv 32 -> 64), slot B 1 row at 255, slot C 9 rows from 250 (across 256, and
    off >> 3 changes the placement): a row reads the K / V its slot's earlier rows stored in the same pass, from
    the cache, its own position included; garbage past each slot's last row; one row alone with the taps"""
    ctx = 320
    fails = []
    for name in ("cancel_kq", "cancel_kqv", "underflow", "benign", "normal"):
        b = _slot_rows_batch(name, H, Hkv, hd, ctx, [(29, 5), (255, 1), (250, 9)])
        fails += _check(b, _run(b, 3, dsplit, taps=False), f"slot rows H {H} hd {hd} dsplit {dsplit} {name} T 15")
        for first in (31, 287):
            b = _slot_rows_batch(name, H, Hkv, hd, ctx, [(first, 1)])
            fails += _check(b, _run(b, 3, dsplit), f"slot rows H {H} hd {hd} dsplit {dsplit} {name} T 1")
    _assert_none(fails)


# ---- refusals ------------------------------------------------------------------------------------------

def _tiny(H, Hkv, hd, ctx, n=1):
    """n rows at position 1 on n slots of arbitrary (possibly unsupported) geometry; no oracle"""
    b = Batch(H, Hkv, hd, ctx, True)
    rng = np.random.default_rng(3)
    kvw = Hkv * hd
    b.qkv = rng.standard_normal((n, (H + 2 * Hkv) * hd)).astype(np.float32)
    b.pos, b.slot, b.tag, b.ref = [1] * n, list(range(n)), ["tiny"] * n, []
    b.kc0 = A._garbage(rng, (n, ctx, kvw))
    b.vc0 = A._garbage(rng, (n, kvw, ctx))
    return b


def _refused(b, o, message):
    assert o["r"] != 0 and message in o["why"], (o["r"], o["why"], message)
    assert (o["out"] == OUT_S).all() and np.array_equal(o["kc"], b.kc0) and np.array_equal(o["vc"], b.vc0)
    for k, s in (("w", W_S), ("p", P_S), ("act", ACT_S), ("da", DA_S), ("q8k", Q8K_S)):
        assert o[k] is None or (o[k] == s).all(), k


@gpu
def test_refusals_start_nothing():
    """a shape or a pass a launcher does not serve: non-zero with the launcher's message; out, the caches and
    every optional output keep what the caller put there"""
    per_head = "attn_decode: unsupported shape for the per-head form"
    for (H, Hkv, hd, ctx, ds), kw in [((2, 1, 512, 64, 1), {}), ((2, 1, 48, 64, 1), {}), ((2, 1, 64, 64, 4), {}),
                                      ((2, 1, 128, 64, 8), {}), ((2, 1, 64, 48, 1), {}), ((3, 2, 64, 64, 1), {}),
                                      ((2, 1, 256, 64, 2), dict(q8k=True)), ((2, 1, 128, 64, 1), dict(q8k=True))]:
        b = _tiny(H, Hkv, hd, ctx)
        _refused(b, _run(b, 0, ds, **kw), per_head)
    b = _tiny(4, 2, 256, 512)
    _refused(b, _run(b, 1, nwg=3), "attn_decode: unsupported shape or missing scratch")
    _refused(b, _run(b, 1, q8k=True), "attn_decode: unsupported shape or missing scratch")
    b = _tiny(8, 1, 256, 16384)
    _refused(b, _run(b, 1), "attn_decode: context too long for the LDS image")  # G 8: 8 * 16384 * 2 B of P16 alone
    for form, who in ((2, "attn_slots"), (3, "attn_slot_rows")):
        b = _tiny(2, 1, 64, 32, 65)
        for R in (0, 65):
            _refused(b, _run(b, form, taps=False, R=R), who + ": unsupported shape for the per-head form, or a pass outside [1, 64] rows")
        b = _tiny(2, 1, 64, 32)
        _refused(b, _run(b, form, img=True), who + ": unsupported shape")
        _refused(b, _run(b, form, 4), who + ": unsupported shape")
        b = _tiny(2, 1, 64, 16384)
        _refused(b, _run(b, form), who + ": context too long for the LDS image")


@gpu
def test_bad_arguments_are_refused_by_the_entry():
    entry = "gemma_test_attn_decode_rows: "
    b = _tiny(2, 1, 64, 32, 2)
    b.pos = [1, 32]
    _refused(b, _run(b, 0), entry + "a row's position outside")
    b.pos, b.slot = [1, 2], [0, 2]
    _refused(b, _run(b, 0), entry + "a row's position outside")
    b.slot = [1, 1]
    _refused(b, _run(b, 2, taps=False), entry + "form 2 needs a distinct slot per row")
    b.slot = [0, 1]
    _refused(b, _run(b, 2), entry + "the taps are indexed by head only")
    _refused(b, _run(b, 3), entry + "the taps are indexed by head only")
    b.pos, b.slot = [1, 3], [0, 0]
    _refused(b, _run(b, 3, taps=False), entry + "form 3 needs a slot's rows at consecutive positions")
    _refused(b, _run(b, 4), entry + "bad arguments")
    _refused(b, _run(b, 0, R=0), entry + "bad arguments")
