"""The penalty kernels alone (penalty.hip through gemma_test_penalize) against the rule of
include/gemma_hpc.h restated in numpy float32: the penalised rows bit for bit, the restored rows equal
to the input bit for bit, the save count the number of distinct in-range window tokens.

Window lengths sit at the edges of the kernel's structure: one element, one pair, around a wave (64),
around the workgroup (1024), past a power of two (4097) and the full LDS array (8192); each is reached
by last_n with a longer history and by a window clipped at index 0."""
import numpy as np
import pytest

import gemma_hip as G

pytestmark = pytest.mark.gpu

V = 8192 + 37
LENGTHS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 8192]
PARAMS = [(1.1, 0.0, 0.0), (1.0, 0.5, 0.25), (1.3, -0.5, 0.1), (0.8, 0.0, 0.0)]  # repeat, presence, frequency
KINDS = ["one", "distinct", "random", "out_of_range"]
PLANTS = np.array([0.0, -0.0, 1e-40, -1e-40, -np.inf, 60.0], dtype=np.float32)  # 60: the row maximum


def penalise(row, hist, p, repeat, presence, frequency, last_n):
    """(l', distinct in-range window tokens) of the row that processed index p: the rule, line for line"""
    f = np.float32
    win = np.asarray(hist[max(0, p + 1 - last_n):p + 1], dtype=np.int64)
    t, c = np.unique(win[(win >= 0) & (win < row.size)], return_counts=True)
    out, l = row.copy(), row[t]
    with np.errstate(all="ignore"):
        a = np.where(l <= 0, l * f(repeat), l / f(repeat))
        pen = (c.astype(f) * f(frequency)) + f(presence)
        out[t] = a - pen
    return out, t.size


def history(kind, H, n, rng):
    if kind == "one":
        return np.full(H, 7, dtype=np.int32)
    if kind == "distinct":
        return ((np.arange(H) + int(rng.integers(V))) % V).astype(np.int32)
    h = rng.integers(0, min(V, n // 3 + 2), H).astype(np.int32)  # about three occurrences a token
    if kind == "out_of_range":
        h[rng.random(H) < 0.2] = -1
        h[rng.random(H) < 0.2] = V
        h[rng.random(H) < 0.05] = 2 ** 31 - 1
    return h


def check(rows, hist, pos, prm, last_n):
    pen, res, n_saved = G.test_penalize(rows, hist, pos, prm + (last_n,))
    for r in range(len(rows)):
        ref, distinct = penalise(rows[r], hist[r], int(pos[r]), *prm, last_n)
        assert np.array_equal(pen[r].view(np.uint32), ref.view(np.uint32)), (r, np.flatnonzero(pen[r] != ref)[:8])
        assert n_saved[r] == distinct, (r, n_saved[r], distinct)
    assert np.array_equal(res.view(np.uint32), rows.view(np.uint32))


def planted(rng, hist, pos, last_n, salt):
    rows = rng.standard_normal((len(pos), V)).astype(np.float32) * np.float32(4.0)
    for r, p in enumerate(pos):
        win = hist[r][max(0, p + 1 - last_n):p + 1]
        u = np.unique(win[(win >= 0) & (win < V)])[:len(PLANTS)]
        rows[r, u] = PLANTS[(np.arange(u.size) + r + salt) % len(PLANTS)]
    return rows


@pytest.mark.parametrize("prm", PARAMS, ids=lambda p: "r%g_p%g_f%g" % p)
@pytest.mark.parametrize("clipped", [False, True], ids=["last_n", "clipped"])
@pytest.mark.parametrize("n", LENGTHS)
def test_window(n, clipped, prm):
    rng = np.random.default_rng(n * 8 + clipped)
    H = 2 * n + 80
    # the window is n long: by last_n under a longer history, or cut at index 0 under a larger last_n
    last_n = min(n + 5, G.PENALTY_MAX_LAST_N) if clipped else n
    pos = np.array([n - 1, n - 1, n // 2] if clipped else [n + 5, n + 70, 2 * n + 1], dtype=np.int32)
    for salt, kind in enumerate(KINDS):
        hist = np.stack([history(kind, H, n, rng) for _ in pos])
        check(planted(rng, hist, pos, last_n, salt), hist, pos, prm, last_n)


def test_64_rows():
    rng = np.random.default_rng(64)
    pos = rng.integers(0, 300, 64).astype(np.int32)
    hist = np.stack([history(KINDS[r % 4], 300, 65, rng) for r in range(64)])
    check(planted(rng, hist, pos, 65, 0), hist, pos, PARAMS[2], 65)


def test_off_and_refused():
    rng = np.random.default_rng(1)
    pos = np.array([10, 20, 30], dtype=np.int32)
    hist = np.stack([history("random", 64, 30, rng) for _ in pos])
    rows = planted(rng, hist, pos, 64, 0)
    for off in (None, (1.0, 0.0, 0.0, 64)):
        pen, res, n_saved = G.test_penalize(rows, hist, pos, off)
        assert np.array_equal(pen.view(np.uint32), rows.view(np.uint32)) and not n_saved.any()
        assert np.array_equal(res.view(np.uint32), rows.view(np.uint32))
    for bad, word in (((0.0, 0.0, 0.0, 64), "repeat"), ((1.1, 0.0, 0.0, 0), "last_n"), ((1.1, 0.0, 0.0, 8193), "last_n"),
                      ((1.1, float("nan"), 0.0, 64), "finite")):
        out = (np.full_like(rows, 7.0), np.full_like(rows, 7.0), np.full(3, 7, dtype=np.int32))
        with pytest.raises(RuntimeError, match=word):
            G.test_penalize(rows, hist, pos, bad, out=out)
        assert all((o == 7).all() for o in out)
