"""numpy restatement of the engine's sampling rule (include/gemma_hpc.h, DESIGN.md §5b″): a helper
for the sampler tests, not a test.

    K = min(top_k, V), top_k == 0 -> min(1024, V)
    candidates c_0 .. c_{K-1}: the first K entries under "larger logit, then smaller index" (np.lexsort;
        float compare, so -0.0 ties +0.0)
    w_i = exp((f64(l[c_i]) - f64(l[c_0])) / f64(temperature)), C = cumsum(w), W = C[K-1]
    m = K when top_p == 1, else the smallest i + 1 with C_i >= f64(top_p) * W   (top_p is an f32)
    u = (mix(seed + (p + 1) * 0x9E3779B97F4A7C15) >> 11) * 2^-53   (splitmix64, mod 2^64)
    r = u * C[m-1]; the token is c_j for the smallest j < m with C_j > r, else j = m - 1

Every draw also carries an `ambiguous` flag: true when some C_i lies within 1e-9 * C[m-1] of r, or
(top_p < 1) within 1e-9 * W of top_p * W.  An f64 exp and a reordered sum of <= 1024 terms move a
prefix sum by parts in 1e-13, so only a flagged draw may legitimately differ on the device."""
import numpy as np

MAX_K = 1024
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
MARGIN = 1e-9


# the draw cases the CPU and the GPU tests share: (V, top_k, temperature, top_p, sd, positions)
DRAW_SEED = 12345
DRAW_CASES = [(4096, 40, 0.8, 0.95, 1.0, 4096), (1000, 64, 1.0, 1.0, 2.0, 4096), (4096, 40, 1.0, 0.95, 0.02, 4096),
              (256000, 1024, 1.5, 0.9, 3.0, 256)]


def make_row(seed, V, sd):
    return (np.random.default_rng(seed).standard_normal(V) * sd).astype(np.float32)


def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def uniform(seed, p):
    """u in [0, 1) for sequence index p"""
    return (mix((seed + (p + 1) * GOLDEN) & M64) >> 11) * 2.0 ** -53


def n_candidates(top_k, V):
    return min(top_k if top_k > 0 else MAX_K, V)


def candidates(row, top_k):
    """candidate ids in order (int64 [K])"""
    row = np.asarray(row, dtype=np.float32)
    K = n_candidates(top_k, row.size)
    # lexsort: last key is primary.  -row ascending = logit descending (-0.0 == +0.0 as floats),
    # ties by the index ascending
    order = np.lexsort((np.arange(row.size), -row.astype(np.float64)))
    return order[:K]


class Table:
    """what does not depend on the position: candidates, prefix sums, the top-p cut"""

    def __init__(self, row, temperature, top_k, top_p):
        row = np.asarray(row, dtype=np.float32)
        self.cand = candidates(row, top_k)
        l = row[self.cand].astype(np.float64)
        with np.errstate(over="ignore", under="ignore"):
            w = np.exp((l - l[0]) / np.float64(np.float32(temperature)))
        self.C = np.cumsum(w)
        self.W = self.C[-1]
        self.K = self.cand.size
        tp = np.float32(top_p)
        self.cut_ambiguous = False
        if tp == np.float32(1.0):
            self.m = self.K
        else:
            thr = np.float64(tp) * self.W
            self.m = int(np.searchsorted(self.C, thr, side="left")) + 1  # first C_i >= thr
            self.m = min(self.m, self.K)
            self.cut_ambiguous = bool((np.abs(self.C - thr) <= MARGIN * self.W).any())
        self.probs = np.diff(np.concatenate(([0.0], self.C[:self.m]))) / self.C[self.m - 1]

    def draw(self, seed, p):
        """(token, ambiguous) at sequence index p"""
        Cm = self.C[:self.m]
        r = uniform(seed, p) * Cm[-1]
        j = int(np.searchsorted(Cm, r, side="right"))  # first C_j > r
        j = min(j, self.m - 1)
        amb = self.cut_ambiguous or bool((np.abs(Cm - r) <= MARGIN * Cm[-1]).any())
        return int(self.cand[j]), amb


def sample(row, temperature, top_k, top_p, seed, p):
    """(token, n_kept m, ambiguous, candidates) for one row at sequence index p"""
    t = Table(row, temperature, top_k, top_p)
    tok, amb = t.draw(seed, p)
    return tok, t.m, amb, t.cand
