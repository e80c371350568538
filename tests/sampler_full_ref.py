"""numpy restatement of the whole-vocabulary sampling rule (top_k == GEMMA_TOP_K_ALL; include/gemma_hpc.h,
DESIGN.md §5b″): a helper for the sampler tests, not a test.

    q_i = (u64) floor(exp((f64(l_i) - f64(l_max)) / f64(temperature)) * 2^40), W = sum q_i
    top_p == 1: every entry is kept.  Else P = max((u64)(f64(top_p) * f64(W)), 1) and the nucleus is
        every entry whose logit is >= the largest logit level (np.unique; -0.0 == +0.0) at which the
        mass of that level and all above it reaches P: a run of equal logits is kept whole
    M = the kept mass, u = sampler_ref.uniform(seed, p), r = min((u64)(u * f64(M)), M - 1)
    the token is the smallest kept index j whose prefix sum of kept masses, in index order, is > r

The device's exp may differ from numpy's by an ulp, so a q_i may differ by one unit and any sum by at
most V units.  A draw is flagged `ambiguous` when r lies within 2 V units of a kept prefix sum, or
(top_p < 1) when a level's cumulative mass lies within 2 V units of P: only a flagged draw may
legitimately differ on the device."""
import numpy as np

from sampler_ref import DRAW_SEED, make_row, uniform  # noqa: F401  (the tests take them from here)

TOP_K_ALL = 0x7FFFFFFF
ONE = 1 << 40

# the draw cases the CPU and the GPU tests share: (V, temperature, top_p, sd, positions)
DRAW_CASES = [(256000, 1.0, 1.0, 1.0, 512), (256000, 0.7, 0.9, 3.0, 512), (4097, 1.0, 0.95, 1.0, 4096),
              (1000, 1.5, 1.0, 2.0, 4096), (5000, 1.0, 0.95, 0.02, 4096), (63, 0.8, 0.5, 1.0, 4096)]


class Table:
    """what does not depend on the position: masses, the nucleus, prefix sums in index order"""

    def __init__(self, row, temperature, top_p):
        row = np.asarray(row, dtype=np.float32)
        l = row.astype(np.float64) + 0.0  # -0.0 + 0.0 = +0.0
        self.V = row.size
        self.margin = 2 * self.V
        with np.errstate(over="ignore", under="ignore"):
            q = np.floor(np.exp((l - l.max()) / np.float64(np.float32(temperature))) * ONE).astype(np.int64)
        keep = np.ones(self.V, dtype=bool)
        self.cut_ambiguous = False
        tp = np.float32(top_p)
        if tp != np.float32(1.0):
            P = max(int(np.float64(tp) * np.float64(int(q.sum()))), 1)
            levels, inv = np.unique(l, return_inverse=True)
            mass = np.zeros(levels.size, dtype=np.int64)
            np.add.at(mass, inv, q)
            above = np.cumsum(mass[::-1])  # above[k]: the mass of the k + 1 highest levels
            k = int(np.searchsorted(above, P, side="left"))  # the first with above >= P
            keep = l >= levels[::-1][min(k, levels.size - 1)]
            self.cut_ambiguous = bool((np.abs(above - P) <= self.margin).any())
        self.n_kept = int(keep.sum())
        self.C = np.cumsum(np.where(keep, q, 0))
        self.M = int(self.C[-1])
        self.steps = self.C[keep]  # the kept prefix sums

    def draw(self, seed, p):
        """(token, ambiguous) at sequence index p"""
        r = min(int(uniform(seed, p) * float(self.M)), self.M - 1)
        j = int(np.searchsorted(self.C, r, side="right"))  # the first C_j > r: a kept entry of mass > 0
        k = int(np.searchsorted(self.steps, r, side="left"))
        near = self.steps[max(k - 1, 0):k + 1]
        return j, self.cut_ambiguous or bool((np.abs(near - r) <= self.margin).any())
