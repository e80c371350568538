"""attention kernel time of one pass: argv = att_mx(0|2) shape(a|b).  a: T 512 at p0 2048; b: T 8 at p0 2560.
Set-up passes run under att_mx 1 below 2556 keys (k_attn_mx: another kernel name); 4 measured passes (the first is warm-up)."""
import sys, os
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, "gemma.ggml_amd", "python")); sys.path.insert(0, os.path.join(R, "tests"))
import gemma_hip as G
import oracle_ctypes as O
form, shape = int(sys.argv[1]), sys.argv[2]
S = dict(O.GEMMA_2B, n_layer=2, n_vocab=8192)
p0, T = (2048, 512) if shape == "a" else (2560, 8)
prompt = [int(t) for t in O.make_prompt(p0 + T, S["n_vocab"])]
e = G.Engine(S, n_ctx=8192, device=0)
e.begin(prompt)
e.prefill_next(2048)
if shape == "b":
    e.prefill_next(479)
    e.set_option("att_mx", 1 if form == 0 else 0)  # 33 rows past k_attn_mx's limit through the form that is not measured
    e.prefill_next(33)
assert e.pos() == p0, e.pos()
e.set_option("att_mx", form)
for i in range(4):
    e.prefill_next(T)
    assert e.pos() == p0 + T
    e.extend(prompt[p0:], keep=p0)
e.close()
print("done", form, shape)
