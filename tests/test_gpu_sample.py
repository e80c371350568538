"""The on-device sampler's kernels (csrc/sample.hip) at the op level, through gemma_test_sample,
against the numpy restatement of the rule (tests/sampler_ref.py).

Candidates (the exact top-K under "larger logit, then smaller index") are compared by integer
equality, no tolerance.  Draws and the top-p cut are compared wherever the reference does not flag the
draw as ambiguous (a prefix sum within 1e-9 of the threshold); the flagged share is bounded and, for
these inputs, zero (tests/test_sampler_ref.py re-checks that on the CPU).  Shapes: one element, below
a wave, no multiple of 64 / 256, one and several workgroups, Gemma's vocabulary; rows whose ties
straddle the K boundary and rows that push more entries into the boundary bin than the tail
workgroup's LDS array holds (the radix-select path)."""
import functools

import numpy as np
import pytest

import gemma_hip as G
import sampler_ref as R

pytestmark = pytest.mark.gpu


def _smp(T=1.0, K=0, top_p=1.0, seed=R.DRAW_SEED):
    return dict(temperature=T, top_k=K, top_p=top_p, seed=seed)


def _check_candidates(row, top_k):
    ref = R.candidates(row, top_k)
    _, cand, n_cand, _ = G.test_sample(row, _smp(K=top_k), [0])
    K = R.n_candidates(top_k, row.size)
    assert n_cand[0] == K == ref.size
    assert np.array_equal(cand[0, :K], ref), (np.nonzero(cand[0, :K] != ref)[0][:8], cand[0, :8], ref[:8])
    assert (cand[0, K:] == -1).all()


@functools.lru_cache(maxsize=None)
def _row(V, sd=1.0, seed=7):
    r = R.make_row(seed, V, sd)
    r.setflags(write=False)
    return r


@pytest.mark.parametrize("top_k", [1, 2, 40, 64, 1000, 1024, 0])
@pytest.mark.parametrize("V", [1, 63, 1000, 4096, 256000])
def test_candidates_exact(V, top_k):
    _check_candidates(_row(V), top_k)  # top_k > V clamps


@pytest.mark.parametrize("top_k", [40, 1024])
@pytest.mark.parametrize("V", [4096, 20000])
def test_ties_across_the_k_boundary(V, top_k):
    """8 distinct values: the K-th candidate lies inside a run of equal logits (V = 20000: the run is
    longer than the tail's LDS array, so the radix select narrows it)"""
    row = np.clip(np.round(_row(V, 1.5, seed=11)), -3.5, 3.5).astype(np.float32)
    _check_candidates(row, top_k)


@pytest.mark.parametrize("V,top_k", [(300, 40), (5000, 40), (256000, 1024)])
def test_all_equal_row(V, top_k):
    row = np.full(V, 0.25, dtype=np.float32)
    _, cand, n_cand, _ = G.test_sample(row, _smp(K=top_k), [3])
    assert n_cand[0] == top_k and list(cand[0, :top_k]) == list(range(top_k))


def test_signed_zeros_tie():
    row = np.zeros(700, dtype=np.float32)
    row[::2] = -0.0
    row[333] = 1.0
    _check_candidates(row, 40)
    _, cand, _, _ = G.test_sample(row, _smp(K=40), [0])
    assert list(cand[0, :40]) == [333] + list(range(39))


def test_minus_inf_candidates_come_last_and_are_never_drawn():
    V, K = 512, 300
    row = _row(V).copy()
    row[::2] = -np.inf  # 256 finite entries, K = 300
    _check_candidates(row, K)
    n = 512
    toks, cand, _, n_kept = G.test_sample(np.broadcast_to(row, (n, V)), _smp(T=5.0, K=K), np.arange(n))
    assert (n_kept == K).all()
    assert np.isfinite(row[toks]).all()
    assert np.array_equal(cand[0, 256:K], np.arange(0, 88, 2))  # the -inf entries, in index order


@pytest.mark.parametrize("case", R.DRAW_CASES, ids=lambda c: f"V{c[0]}-K{c[1]}")
def test_draws_equal_the_reference(case):
    V, K, T, top_p, sd, n_pos = case
    row = R.make_row(R.DRAW_SEED, V, sd)
    t = R.Table(row, T, K, top_p)
    ref = [t.draw(R.DRAW_SEED, p) for p in range(n_pos)]
    ref_tok = np.array([r[0] for r in ref])
    clear = ~np.array([r[1] for r in ref])
    toks, cand, n_cand, n_kept = G.test_sample(np.broadcast_to(row, (n_pos, V)), _smp(T, K, top_p), np.arange(n_pos))
    assert (~clear).sum() <= 1e-3 * n_pos
    assert (n_cand == t.K).all() and (cand[:, :t.K] == t.cand[None, :]).all()
    assert (n_kept[clear] == t.m).all(), (np.unique(n_kept), t.m)
    bad = np.nonzero(clear & (toks != ref_tok))[0]
    assert bad.size == 0, (bad[:8], toks[bad[:8]], ref_tok[bad[:8]])
    assert len(set(toks.tolist())) > 8  # it does sample


def test_extremes():
    V = 4096
    row = _row(V, 2.0).copy()
    am = int(np.argmax(row))
    row[am] += np.float32(1.0)  # a gap of >= 1: at T = 1e-3 every other weight is exp(-1000) = 0
    pos = np.arange(256)
    rows = np.broadcast_to(row, (256, V))
    toks, _, _, _ = G.test_sample(rows, _smp(T=1e-3, K=40), pos)  # weights underflow: argmax
    assert (toks == am).all()
    toks, _, _, n_kept = G.test_sample(rows, _smp(T=1.0, K=40, top_p=1e-6), pos)  # m = 1
    assert (n_kept == 1).all() and (toks == am).all()
    toks, cand, _, _ = G.test_sample(rows, _smp(T=100.0, K=40), pos)  # nearly uniform over the 40
    t = R.Table(row, 100.0, 40, 1.0)
    assert np.array_equal(toks, [t.draw(R.DRAW_SEED, int(p))[0] for p in pos])
    assert len(set(toks.tolist())) >= 30 and t.probs.max() < 1.1 / 40
    # the draw is keyed by (seed, p): equal keys in one call give equal tokens, other keys other u
    toks, _, _, _ = G.test_sample(rows[:6], _smp(T=100.0, K=40), [5, 5, 9, 9, 5, 9])
    assert toks[0] == toks[1] == toks[4] and toks[2] == toks[3] == toks[5]
    assert R.uniform(R.DRAW_SEED, 5) != R.uniform(R.DRAW_SEED, 9)
    a, _, _, _ = G.test_sample(rows[:64], _smp(T=100.0, K=40, seed=1), pos[:64])
    b, _, _, _ = G.test_sample(rows[:64], _smp(T=100.0, K=40, seed=2), pos[:64])
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("smp,field", [(_smp(K=-1), "top_k"), (_smp(K=1025), "top_k"), (_smp(top_p=0.0), "top_p"),
                                       (_smp(top_p=1.5), "top_p"), (_smp(T=float("nan")), "temperature")])
def test_refusals_name_the_field(smp, field):
    with pytest.raises(RuntimeError, match=field):
        G.test_sample(_row(63), smp, [0])


def test_refuses_an_empty_vocabulary():
    L = G.lib()
    s = G.GemmaSampler(1.0, 0, 1.0, 0)
    x = np.zeros(4, dtype=np.float32)
    pos = np.zeros(1, dtype=np.int32)
    assert L.gemma_test_sample(x.ctypes.data, 1, 0, s, pos.ctypes.data, None, None, None, None) == -1
    assert "n_vocab" in G.last_error()
