"""CPU: gemma_lookup_draft (a host function of libgemma_hip.so: no GPU call) against a Python
restatement of the rule in include/gemma_hpc.h, on random sequences over a small alphabet (where
n-grams repeat) and on crafted cases."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))

import gemma_hip as G  # noqa: E402


def rule(seq, ngram_max, k):
    """for g = min(ngram_max, n - 1) .. 1: the largest s < n - g with seq[s:s+g] == seq[n-g:]; the
    first g with a match wins; the draft is seq[s+g : min(s+g+k, n)]"""
    seq = list(seq)
    n = len(seq)
    for g in range(min(ngram_max, n - 1), 0, -1):
        for s in range(n - g - 1, -1, -1):
            if seq[s:s + g] == seq[n - g:]:
                return seq[s + g:min(s + g + k, n)]
    return []


def test_random_sequences_match_the_rule():
    rng = np.random.default_rng(7)
    some_draft = 0
    for _ in range(200):
        n = int(rng.integers(1, 41))
        seq = [int(t) for t in rng.integers(0, 4, n)]
        ngram_max, k = int(rng.integers(1, 5)), int(rng.integers(1, 8))
        want = rule(seq, ngram_max, k)
        assert G.lookup_draft(seq, ngram_max, k) == want, (seq, ngram_max, k)
        some_draft += bool(want)
    assert some_draft > 100  # the alphabet is small enough that most sequences have a match


def test_no_match_returns_nothing():
    assert G.lookup_draft([1, 2, 3, 4, 5], 3, 4) == []


def test_single_token():
    assert G.lookup_draft([9], 3, 4) == []


def test_longest_ngram_wins_over_a_more_recent_shorter_match():
    #      0  1  2  3  4  5  6  7  8
    seq = [1, 2, 3, 7, 9, 3, 8, 2, 3]
    # g = 2: (2, 3) occurs at s = 1 -> draft from index 3; g = 1 alone would take the 3 at s = 5 -> 8
    assert G.lookup_draft(seq, 2, 2) == [7, 9]
    assert G.lookup_draft(seq, 1, 2) == [8, 2]


def test_most_recent_match_wins_within_one_g():
    seq = [5, 1, 5, 2, 5, 3, 5]
    assert G.lookup_draft(seq, 1, 1) == [3]
    assert G.lookup_draft(seq, 1, 3) == [3, 5]  # and the draft stops at the end of the sequence


def test_draft_is_truncated_at_the_sequence_end():
    seq = [4, 6, 4]
    assert G.lookup_draft(seq, 3, 7) == [6, 4]
    assert G.lookup_draft([2, 2], 3, 7) == [2]


def test_bad_arguments():
    for ngram_max, k in ((0, 3), (2, 0), (2, 8)):
        with pytest.raises(ValueError, match="gemma_lookup_draft"):
            G.lookup_draft([1, 2, 1], ngram_max, k)
