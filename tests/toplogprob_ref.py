"""numpy restatement of the alternatives' rule (include/gemma_hpc.h at gemma_engine_set_top_logprobs):
a helper for the top-logprob tests, not a test.

Entry i of a row has the key (ordered bits of l[i], ~i); the alternatives are the min(n, V) entries
with the largest keys, descending: larger value first, -0 below +0, the smaller index first among
equal bits.  Each carries logprob_ref.logprob(row, i); entries past min(n, V) are token -1, value NaN."""
import numpy as np

import logprob_ref


def ordered_bits(row):
    u = np.asarray(row, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def top(row, n):
    """(tokens i32 [n], lps f64 [n]) of one row"""
    l = np.asarray(row, dtype=np.float32)
    order = np.lexsort((np.arange(l.size), -ordered_bits(l).astype(np.int64)))[:n]  # last key is the primary one
    tok = np.full(n, -1, dtype=np.int32)
    lps = np.full(n, np.nan, dtype=np.float64)
    tok[:order.size] = order
    lps[:order.size] = [logprob_ref.logprob(l, t) for t in order]
    return tok, lps


def tops(rows, n):
    """top() of every row: (tokens [R][n], lps [R][n])"""
    both = [top(r, n) for r in np.atleast_2d(rows)]
    return np.array([b[0] for b in both]), np.array([b[1] for b in both])


def close(got, ref):
    """elementwise: both NaN (padding), or logprob_ref.close"""
    return (np.isnan(got) & np.isnan(ref)) | logprob_ref.close(got, ref)
