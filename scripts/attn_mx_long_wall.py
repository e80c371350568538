"""wall time of an 8,000-token prompt on Gemma-2B, n_ctx 8192: chunks of 512 through prefill_next against 8,000 steps"""
import sys, os, time, statistics
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, "gemma.ggml_amd", "python")); sys.path.insert(0, os.path.join(R, "tests"))
import gemma_hip as G
import oracle_ctypes as O
S = dict(O.GEMMA_2B)
N = 7800
prompt = [int(t) for t in O.make_prompt(N, S["n_vocab"])]
e = G.Engine(S, n_ctx=7904, device=0)
def chunks():
    e.extend(prompt, keep=0) if e.pos() else e.begin(prompt)
    t = time.perf_counter()
    while e.pos() < N:
        e.prefill_next(min(512, N - e.pos()))
    tok = int(e.tokens()[-1])
    return time.perf_counter() - t, tok
def steps():
    e.extend(prompt, keep=0) if e.pos() else e.begin(prompt)
    t = time.perf_counter()
    e.step(N, use_graph=True)
    tok = int(e.tokens()[-1])
    return time.perf_counter() - t, tok
for name, fn, reps in (("chunks of 512", chunks, 5), ("7800 steps", steps, int(sys.argv[1]) if len(sys.argv) > 1 else 5)):
    fn()
    r = [fn() for _ in range(reps)]
    ts = sorted(x[0] for x in r)
    print(f"{name}: median {statistics.median(ts):.3f} s of {reps} (min {ts[0]:.3f} max {ts[-1]:.3f}); next token {r[0][1]}", flush=True)
e.close()
