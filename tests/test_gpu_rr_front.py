"""The round-pipelined matvec (csrc/matvec_rr.hip) through every kernel it instantiates, bit for bit against
the oracle's pieces, in the manner of test_gpu_kernarg_args.py (whose launcher and references these cases use).

The kernel has two forms: a refilled ring (D < NR, the down kernels) runs the loader waves and the carrier wave
on separate straight-line paths, with E of the ring's D rounds issued in front of the activation image; a
one-shot ring runs one joined path.  E is a constant per class of kernel: every E the build instantiates is run
here, since every kernel is.  So the cases are the kernels:
  * Q4_0 and Q8_0;
  * every (prologue, epilogue) pair the dispatcher instantiates;
  * every round count NR in {1, 2, 3, 8, 12, 16} at the smallest K that gives it (K = 2048 NR for Q4_0,
    1024 NR for Q8_0): the one-shot ring (NR <= D), the refilled rings of depth 4, 6 and 8, and the image
    prologue's Gemma-7B shape (Q4_0, NR 12), whose image needs more than two items per thread;
  * 20 rows: two full row tiles and a ragged one (4 rows: the residual's clamped address);
  * one and two columns, the columns apart by more than a row."""
import ctypes as C

import numpy as np
import pytest

import oracle_ctypes as O
import test_gpu_kernarg_args as KA

gpu = pytest.mark.gpu

PRO_Q8 = 2
PAIRS = [(PRO_Q8, KA.EPI_STORE), (KA.PRO_NORM, KA.EPI_STORE), (KA.PRO_EMBED, KA.EPI_STORE), (KA.PRO_F32, KA.EPI_ADD),
         (KA.PRO_IMG, KA.EPI_ADD), (KA.PRO_F32, KA.EPI_STORE)]
PAIR_IDS = ["q8", "norm", "embed", "f32_add", "img_add", "f32"]
ROWS = 20


def _run_q8(wtype, rows, K, ncols, seed):
    """PRO_Q8: the activation as ggml block_q8_0 rows, the columns x_stride bytes apart"""
    G, L = KA._entry()
    rng = np.random.default_rng(seed)
    W = KA._weights(rng, wtype, rows, K)
    q8 = [O.quantize(rng.standard_normal(K).astype(np.float32)[None], "q8_0")[0] for _ in range(ncols)]
    row_bytes = K // 32 * 34
    x_stride = row_bytes + 34 if ncols > 1 else row_bytes
    y_stride = rows + 5 if ncols > 1 else rows
    xbuf = np.zeros((ncols - 1) * x_stride + row_bytes, dtype=np.uint8)
    for c in range(ncols):
        xbuf[c * x_stride: c * x_stride + row_bytes] = np.ascontiguousarray(q8[c]).view(np.uint8).ravel()
    y = np.zeros((ncols - 1) * y_stride + rows, dtype=np.float32)
    t = KA.MatvecArgs(type=wtype, ks=KA.KS_RR, pro=PRO_Q8, epi=KA.EPI_STORE, ncols=ncols, grid=1, rows=rows, K=K,
                      W=W.ctypes.data, x=xbuf.ctypes.data, x_stride=x_stride, y_stride=y_stride, y=y.ctypes.data,
                      eps=KA.EPS, emb_scale=1.0)
    assert L.gemma_test_matvec(C.byref(t)) == 0, G.last_error()
    wdata = np.ascontiguousarray(np.stack(q8))
    ref = O.mul_mat(W, wtype, rows, W.shape[1], K, wdata, wdata.shape[1], ncols)
    for c in range(ncols):
        got = y[c * y_stride: c * y_stride + rows]
        bad = np.flatnonzero(got.view(np.uint32) != ref[c].view(np.uint32))
        assert bad.size == 0, f"column {c}: {bad.size} of {rows} rows differ, first {bad[:5]}"
        if c + 1 < ncols:  # the gap between columns stays untouched
            assert not y[c * y_stride + rows: (c + 1) * y_stride].any()


@gpu
@KA.TYPES
@KA.NCOLS
@pytest.mark.parametrize("nr", [1, 2, 3, 8, 12, 16], ids=lambda n: f"nr{n}")
@pytest.mark.parametrize("pro,epi", PAIRS, ids=PAIR_IDS)
def test_rr_every_kernel(wtype, ncols, nr, pro, epi):
    K = (2048 if wtype == O.Q4_0 else 1024) * nr
    seed = 100 * nr + 10 * pro + epi
    if pro == PRO_Q8:
        _run_q8(wtype, ROWS, K, ncols, seed)
    else:
        KA._run(wtype, KA.KS_RR, pro, epi, rows=ROWS, K=K, ncols=ncols, grid=1, seed=seed)
