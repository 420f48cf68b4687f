"""Times the nearest-word lookup (msocr_lexicon_nearest) beside the beam decode it runs behind (dev tool).
  python tools/nearest_time.py [--repeats N] [--k K]
For B = 1920 and 7680 rows and lexicons of 1 000 and 100 000 seeded random words (lengths 1..24, mean about 8, over the 191 symbols),
k = 3, without a bound and with max_distance = 2: per round 5 calls of every variant in turn, the beam decode with the attention-weight
output (msocr_attn_decode in beam mode with alpha_out, 26 steps, at B = 1920) among them for scale; one line per variant with the median and the spread
(max - min) over --repeats rounds (default 7).  Half of the rows are lexicon words with 0..2 random edits, half are independent draws
of the same length distribution (out-of-vocabulary readings).  The results are compared with the host twin on the first 8 rows."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from manuscript_ocr_amd import synth
from manuscript_ocr_amd.recognizers import Lexicon
from manuscript_ocr_amd.recognizers._trba.net import AttnDecoder
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--k", type=int, default=3)
a = ap.parse_args()
STEPS, K = 25, a.k
itos = ["<PAD>", "<SOS>", "<EOS>"] + [chr(0x400 + i) for i in range(191)]


def make_lexicon(n):
    rng = np.random.default_rng(n)
    lens = np.clip(rng.poisson(8, size=n), 1, STEPS - 1)
    t0 = time.perf_counter()
    lex = Lexicon(["".join(itos[i] for i in rng.integers(3, 194, size=m)) for m in lens], itos, STEPS)
    lex.wordlist("cuda")
    print(f"lexicon: {len(lex)} words, {len(lex.word_tok)} tokens, built and uploaded in {time.perf_counter() - t0:.2f} s")
    return lex


def make_rows(lex, B, seed):
    rng = np.random.default_rng(seed)
    ids = np.full((B, STEPS), 2, dtype=np.int32)
    for b in range(B):
        if b % 2 == 0:
            w = int(rng.integers(len(lex)))
            s = lex.word_tok[lex.word_begin[w]:lex.word_begin[w + 1]].tolist()
            for _ in range(int(rng.integers(0, 3))):
                s[int(rng.integers(len(s)))] = int(rng.integers(3, 194))
        else:
            s = rng.integers(3, 194, size=int(np.clip(rng.poisson(8), 1, STEPS - 1))).tolist()
        ids[b, :len(s)] = s
    return ids


variants = {}
sd = synth.trba_state_dict(194, 256, seed=1)
dec = AttnDecoder(sd, 194, 256)
torch.manual_seed(0)
bH, pH = torch.randn(1920, 13, 256, device="cuda"), torch.randn(1920, 13, 256, device="cuda")
aws = torch.empty((1920, 26, 8, 13), dtype=torch.float32, device="cuda")
variants["beam + alpha, B 1920 (for scale)"] = lambda: dec.beam(bH, pH, 26, 8, 0.9, 1.7, 1, 2, None, want_alpha=True, alpha_ws=aws)
for n in (1000, 100000):
    lex = make_lexicon(n)
    for B in (1920, 7680):
        ids = make_rows(lex, B, B + n)
        ids_dev = torch.from_numpy(ids).cuda()
        trun_dev = torch.full((B,), STEPS, dtype=torch.int32, device="cuda")
        for bound in (None, 2):
            got = [t.cpu().numpy() for t in lex.nearest_device(ids_dev[:8], trun_dev[:8], K, bound)]
            want = lex.nearest(ids[:8], None, K, bound)
            assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
            idx = lex.nearest_device(ids_dev, trun_dev, K, bound)[0]
            filled = float((idx[:, 0] >= 0).float().mean())
            name = f"nearest, B {B}, {n} words, k {K}, " + ("no bound" if bound is None else f"max_distance {bound}")
            print(f"{name}: rows with a suggestion {filled:.3f}")
            variants[name] = (lambda lex=lex, i=ids_dev, t=trun_dev, bd=bound: lex.nearest_device(i, t, K, bd))
for fn in variants.values():
    for _ in range(2):
        fn()
torch.cuda.synchronize()
ms = {k: [] for k in variants}
for _rep in range(a.repeats):
    for k, fn in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms[k].append(e0.elapsed_time(e1) / 5)
for k, v in ms.items():
    print(f"{k}: median {statistics.median(v):.3f} ms, spread {max(v) - min(v):.3f} ms over {len(v)} rounds")
