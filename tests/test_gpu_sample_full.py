"""The whole-vocabulary sampler (csrc/sample_full.hip, top_k = TOP_K_ALL) against the numpy restatement
of its rule (tests/sampler_full_ref.py): at the op level through gemma_test_sample / _sample_rows, and
inside the decode step and a batch pass.  Only a draw the reference flags (r, or the top-p target,
within 2 V mass units of a sum: the device's exp may differ by an ulp) may differ."""
import numpy as np
import pytest

import gemma_hip as G
import oracle_ctypes as O
import sampler_full_ref as F

pytestmark = pytest.mark.gpu

ALL, S = G.TOP_K_ALL, F.DRAW_SEED
N_CTX, N_PROMPT = 256, 20


def _smp(T=1.0, top_p=1.0, seed=S, top_k=ALL):
    return dict(temperature=T, top_k=top_k, top_p=top_p, seed=seed)


def _against_reference(row, T, top_p, n_pos, flagged_share=1e-3):
    """n_pos draws of one row on the device against the reference's; returns the device's tokens"""
    V = row.size
    t = F.Table(row, T, top_p)
    ref = [t.draw(S, p) for p in range(n_pos)]
    ref_tok, clear = np.array([r[0] for r in ref]), ~np.array([r[1] for r in ref])
    step = max(1, (1 << 26) // V)  # slabs of at most 256 MiB of logits
    parts = [G.test_sample(np.broadcast_to(row, (min(step, n_pos - p0), V)), _smp(T, top_p), np.arange(p0, min(p0 + step, n_pos)))
             for p0 in range(0, n_pos, step)]
    toks, cand, n_cand, n_kept = (np.concatenate(x) for x in zip(*parts))
    print(f"V {V} T {T} top_p {top_p}: flagged {(~clear).sum()} of {n_pos}, kept {t.n_kept}, distinct {len(set(toks.tolist()))}")
    assert (~clear).sum() <= flagged_share * n_pos
    assert (n_cand == V).all() and (cand == -1).all()
    assert (n_kept[clear] == t.n_kept).all(), (np.unique(n_kept), t.n_kept)
    bad = np.nonzero(clear & (toks != ref_tok))[0]
    assert bad.size == 0, (bad[:8], toks[bad[:8]], ref_tok[bad[:8]])
    return toks


@pytest.mark.parametrize("case", F.DRAW_CASES, ids=lambda c: f"V{c[0]}-T{c[1]}-p{c[2]}")
def test_draws_equal_the_reference(case):
    V, T, top_p, sd, n_pos = case
    toks = _against_reference(F.make_row(S, V, sd), T, top_p, n_pos)
    assert V == 63 or len(set(toks.tolist())) > 8  # it does sample (V = 63: a nucleus of 7)


def test_one_entry():
    toks, _, n_cand, n_kept = G.test_sample(np.array([[-3.0]], np.float32), _smp(0.8, 0.9), [5])
    assert (toks[0], n_cand[0], n_kept[0]) == (0, 1, 1)


@pytest.mark.parametrize("top_p", [0.5, 0.8])
def test_a_cut_inside_a_level_keeps_the_level(top_p):
    V = 20000
    row = np.clip(np.round(F.make_row(11, V, 1.5)), -3.5, 3.5).astype(np.float32)
    t = F.Table(row, 1.0, top_p)
    sizes = np.cumsum([(row == v).sum() for v in np.unique(row)[::-1]])
    assert t.n_kept in sizes.tolist() and not t.cut_ambiguous  # whole levels, the cut not at a level's edge
    _against_reference(row, 1.0, top_p, 1024, flagged_share=0.0)


def test_all_equal_row():
    V, n = 5000, 1024
    toks = _against_reference(np.full(V, 0.25, np.float32), 1.0, 1.0, n, flagged_share=0.0)
    want = [min(int(F.uniform(S, p) * V * F.ONE) // F.ONE, V - 1) for p in range(n)]
    assert toks.tolist() == want


def test_minus_inf_and_far_below_entries_are_never_drawn():
    V, n = 512, 2048
    row = F.make_row(S, V, 1.0)
    row[1::2] = -np.inf
    toks = _against_reference(row, 5.0, 1.0, n)
    assert (toks % 2 == 0).all() and len(set(toks.tolist())) > 8
    row = F.make_row(S, 4096, 2.0)
    am = int(np.argmax(row))
    row[am] += np.float32(1.0)  # a gap of >= 1: at T = 1e-3 every other mass is floor(exp(-1000) * 2^40) = 0
    for top_p in (1.0, 0.9):
        toks, _, _, n_kept = G.test_sample(np.broadcast_to(row, (256, row.size)), _smp(1e-3, top_p), np.arange(256))
        assert (toks == am).all() and (n_kept == (row.size if top_p == 1.0 else 1)).all()


def test_one_launch_set_for_mixed_rows():
    V, n = 4096, 12
    rows = np.stack([F.make_row(100 + r, V, 1.0 + 0.25 * (r % 5)) for r in range(n)])
    pos = [(37 * r + 5) % 2048 for r in range(n)]
    kinds = [None, (1.0, 40, 0.95), (0.9, ALL, 0.9), (1.3, ALL, 1.0)]
    samplers = [None if r % 4 == 0 else kinds[r % 4] + (S + r,) for r in range(n)]
    first = G.test_sample_rows(rows, samplers, pos)
    second = G.test_sample_rows(rows, samplers, pos)  # every workspace was left clean
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    for r, sp in enumerate(samplers):
        if sp is None:
            one = G.test_sample_rows(rows[r], [None], [pos[r]])
        else:
            one = G.test_sample(rows[r], dict(zip(("temperature", "top_k", "top_p", "seed"), sp)), [pos[r]])
        for a, b in zip(one, first):
            assert np.array_equal(a[0], b[r]), (r, sp)
        if sp is not None and sp[1] == ALL:
            t = F.Table(rows[r], sp[0], sp[2])
            tok, amb = t.draw(sp[3], pos[r])
            assert not amb and (first[0][r], first[2][r], first[3][r]) == (tok, V, t.n_kept), r


def _prompt():
    return [int(t) for t in O.make_prompt(N_PROMPT, O.TINY["n_vocab"])]


def _generated(e, prompt, n_gen, smp):
    """n_gen tokens after the prompt, each checked against the reference on that step's own logits"""
    e.begin(prompt)
    lg = e.step(N_PROMPT - 1 + n_gen, want_logits=True)
    hist = [int(t) for t in e.tokens()]
    assert len(hist) == N_PROMPT + n_gen and hist[:N_PROMPT] == prompt
    for i in range(n_gen):
        tok, amb = F.Table(lg[N_PROMPT - 1 + i], smp["temperature"], smp["top_p"]).draw(smp["seed"], N_PROMPT + i)
        assert not amb and hist[N_PROMPT + i] == tok, (i, hist[N_PROMPT:], tok)
    return hist


def test_engine_decode_graph_and_mode_changes():
    prompt, smp = _prompt(), _smp(1.0, 0.95, seed=1)
    e = G.Engine(dict(O.TINY), n_ctx=N_CTX)
    e.set_sampler(**smp)
    assert e.sampler() == (True, dict(temperature=1.0, top_k=ALL, top_p=np.float32(0.95), seed=1))
    h1 = _generated(e, prompt, 16, smp)
    assert len(set(h1[N_PROMPT:])) > 4
    for steps in ((8, 8), (16,)):  # graph replays without logits
        e.begin(prompt)
        e.step(N_PROMPT - 1)
        for n in steps:
            e.step(n)
        assert [int(t) for t in e.tokens()] == h1
    n_graph = e.graph_kernels()
    e.set_sampler(**dict(smp, seed=2, temperature=0.9))  # inside the mode: a copy, the captured graph is kept
    assert e.graph_kernels() == n_graph
    h2 = _generated(e, prompt, 16, dict(smp, seed=2, temperature=0.9))
    assert e.graph_kernels() == n_graph and h2 != h1
    e.set_sampler(**_smp(1.0, 0.95, seed=1, top_k=40))  # the truncated sampler: three launches for six
    e.begin(prompt)
    e.step(N_PROMPT + 3)
    assert e.graph_kernels() == n_graph - 3
    e.set_sampler(**smp)
    assert _generated(e, prompt, 16, smp) == h1 and e.graph_kernels() == n_graph
    e.close()


def test_batch_pass_with_a_whole_vocabulary_slot_and_a_greedy_slot():
    prompt, smp, n = _prompt(), _smp(1.0, 0.95, seed=7), 10
    e = G.Engine(dict(O.TINY), n_ctx=N_CTX)
    want = []
    for sp in (smp, None):
        e.set_sampler(**sp) if sp else e.set_sampler(None)
        e.begin(prompt)
        e.step(N_PROMPT - 1 + n)
        want.append([int(t) for t in e.tokens()])
    assert want[0] != want[1]
    e.batch_open(2)
    e.batch_set_sampler(0, **smp)
    e.batch_set_sampler(1, temperature=0.0)
    assert e.batch_sampler(0)[1]["top_k"] == ALL
    for s in (0, 1):
        e.batch_begin(s, prompt)
    e.batch_step(N_PROMPT - 1 + n)
    for s in (0, 1):
        assert [int(t) for t in e.batch_tokens(s)] == want[s], s
    e.close()
