"""GPU: k_attn_decode_win (attn_decode_win.hip), the split decode attention with its softmax image in windows of
1,024 positions, alone through gemma_test_attn_decode_rows form 1 at the shapes whose resident image does not fit
the LDS (launch_attn_decode picks the windowed form there).  Bit equality against orc_attn_decode_row by the
helpers of tests/test_gpu_attn_decode_rows.py: out, scores, P16, the taps past n_kv, K row and V column pos, every
other cache word, the Q8_0 image; counters zero and error word 0 after every call (its second launch ran on the
counters the first one left)."""
import pytest

import attn_adversary as A
from test_gpu_attn_decode_rows import _check, _refused, _run, _successive, _tiny

pytestmark = pytest.mark.gpu
GEMMA_2B = (8, 1, 256, 8192)
MAIN = ("cancel_kq", "cancel_kqv", "underflow", "normal")
# two successive positions from each start.  Gemma-2B's shape: first window only (staged V, n_kv 256), both sides of
# every window edge and half-window (512k - 1, 512k), n_kv capped at ctx with the V patch in the last window;
# ctx 7936: the first multiple of 32 past the resident form; G 16 at head_dim 64: the index arithmetic at G != 8
STARTS = [(GEMMA_2B, s) for s in [0, 31, 255] + [512 * k - 1 for k in range(1, 16)] + [8190]] + \
         [((8, 1, 256, 7936), s) for s in (7934, 4095)] + [((16, 1, 64, 6144), s) for s in (2047, 4095, 6142)]


def _families(shape, start):
    if shape[0] == 16:
        return ("normal",)
    return A.CASES + ("normal",) if shape == GEMMA_2B and start in (4095, 8190) else MAIN


@pytest.mark.parametrize("shape,start", STARTS, ids=[f"G{s[0] // s[1]}-ctx{s[3]}-from{p}" for s, p in STARTS])
def test_windowed_form_equals_the_oracle(shape, start):
    fails = []
    for name in _families(shape, start):
        b = _successive(name, start, 2, *shape)
        o = _run(b, 1, img=shape[0] // shape[1] <= 8)  # (the image needs 32-dim KQV slices: 256 / G >= 32)
        what = f"windowed {shape} from {start} {name}"
        fails += _check(b, o, what)
        if o["r"] == 0 and (o["sync"].any() or o["err"] != 0):
            fails.append(f"{what}: counters {o['sync'].tolist()} error word {o['err']} after the last launch")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:8])


def test_past_8192_is_refused():
    b = _tiny(8, 1, 256, 8224)
    _refused(b, _run(b, 1, img=True), "attn_decode: context too long for the LDS image")
