"""Log-likelihood and perplexity of a token-id text, scored on the device.

    python scripts/score_text.py --tokens ids.txt (--gguf model.gguf | --shape tiny|gemma2b|'{json}')
                                 [--wtype q4_0|q8_0] [--chunk 512] [--fast] [--check]

The text is fed by chunked prefill_next passes with log-probabilities on (gemma_engine_set_logprobs):
every logits row is scored on the device against the token that follows it, and only the T f64 values
come back.  No logits_all is read.  Token i of the text (i >= 1) has lp[i] = log p(token_i | tokens
before it) under softmax of the raw row; the summed log-likelihood is sum(lp[1..T)) and the perplexity
exp(-mean(lp[1..T))).  Token 0 has no row before it and is not scored.

--tokens: a text file of integer ids separated by white space or commas, or a .npy integer array.
Tokenizing is not done here.  --shape runs synthetic weights of that shape (the test
and benchmark shapes, or a JSON object of n_layer, n_embd, n_head, n_head_kv, head_dim, n_ff, n_vocab).
--fast scores the rows of the MFMA tolerance prefill instead of the exact one.
--check also takes logits_all of the same passes to the host, restates the rule in numpy f64 and
prints the largest |device - numpy| and both perplexities (a test of this script, at small shapes).
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))

import gemma_hip as G  # noqa: E402

SHAPES = {"tiny": dict(n_layer=2, n_embd=512, n_head=2, n_head_kv=1, head_dim=256, n_ff=2048, n_vocab=4096),
          "gemma2b": dict(n_layer=18, n_embd=2048, n_head=8, n_head_kv=1, head_dim=256, n_ff=16384, n_vocab=256000)}
WTYPES = {"q4_0": G.GGML_TYPE_Q4_0, "q8_0": G.GGML_TYPE_Q8_0}


def read_tokens(path):
    if path.endswith(".npy"):
        return [int(t) for t in np.load(path).ravel()]
    return [int(t) for t in open(path).read().replace(",", " ").split()]


def host_logprob(row, t):
    """the rule of include/gemma_hpc.h in numpy f64 (--check)"""
    d = row.astype(np.float64) - np.float64(row.max())
    return d[t] - np.log(np.exp(d).sum())


def score(e, tokens, chunk, exact=True, check=False):
    """(lp [T] f64 with lp[0] = NaN, host restatement [T] or None)"""
    T = len(tokens)
    e.set_logprobs(1)
    e.begin(tokens)
    host = np.full(T, np.nan) if check else None
    while e.pos() < T:
        p0, n = e.pos(), min(chunk, T - e.pos())
        out = e.prefill_next(n, want_all=check, exact=exact)
        if check:
            for r in range(n):
                if p0 + r + 1 < T:
                    host[p0 + r + 1] = host_logprob(out[2][r], tokens[p0 + r + 1])
    return e.logprobs(0, T), host


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tokens", required=True)
    ap.add_argument("--gguf")
    ap.add_argument("--shape")
    ap.add_argument("--wtype", default="q4_0", choices=sorted(WTYPES))
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--fast", action="store_true")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    if (args.gguf is None) == (args.shape is None):
        ap.error("give exactly one of --gguf and --shape")
    tokens = read_tokens(args.tokens)
    T = len(tokens)
    if T < 2 or args.chunk < 1:
        ap.error("the text needs at least 2 tokens and --chunk at least 1")
    n_ctx = (T // 32 + 2) * 32
    if args.gguf:
        e = G.Engine.from_gguf(args.gguf, n_ctx=n_ctx)
    else:
        shape = SHAPES[args.shape] if args.shape in SHAPES else json.loads(args.shape)
        e = G.Engine(shape, n_ctx=n_ctx, wtype=WTYPES[args.wtype])
    lp, host = score(e, tokens, args.chunk, exact=not args.fast, check=args.check)
    e.close()
    if np.isnan(lp[1:]).any():
        raise SystemExit("score_text: tokens %s were not scored" % np.flatnonzero(np.isnan(lp[1:]))[:8])
    res = {"tokens": T, "scored": T - 1, "log_likelihood": float(lp[1:].sum()), "perplexity": float(np.exp(-lp[1:].mean())),
           "path": "fast" if args.fast else "exact", "chunk": args.chunk}
    if args.check:
        res["host_perplexity"] = float(np.exp(-host[1:].mean()))
        res["max_abs_lp_diff"] = float(np.abs(lp[1:] - host[1:]).max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
