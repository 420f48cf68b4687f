"""Times the beam-8 decode launch (all 25 steps, no early exit) for B crops, split-operand form against exact-f32 MFMA (dev tool).
  python tools/attn_time.py [B] [--alpha] [--repeats N] [--general] [--greedy] [--nbest] [--forced] [--lexicon N] [--lm ORDER]
--alpha: with the attention-weight output on (the _alpha entry points, into one preallocated buffer).  --repeats N: N timed repeats
of 5 calls each per form, one line each (default 1).  --general: the general kernel (csrc/attn_general.hip) at the same shape
instead of the matrix-core kernels (net.HOIST_CTX = False; one form, no split / exact comparison).  --greedy: the greedy decode
(26 steps) instead of the beam decode: the matrix-core greedy kernel, or the general one with --general; timings only.
--forced: the forced decode (AttnDecoder.forced along the greedy decode's own ids, 26 steps, the context GEMM included as in greedy)
against the greedy decode with the attention-weight output, alternating: per round 5 calls of one, then 5 of the other, --repeats
rounds (default 1); one line per round and variant, then medians and spread (max - min) over the rounds.  With --general on the
general kernels.
--lexicon N: the beam decode constrained to a lexicon of N seeded random words (lengths 1..25, mean about 8, over the 191 symbols)
against the unconstrained beam decode with the attention-weight output (msocr_attn_decode, beam mode with alpha_out), 26 steps, alternating as
--forced does; medians and spread over --repeats rounds, and their ratio.  With --general on the general kernels.
--lm ORDER: the beam decode fused with a character n-gram language model of that order (a seeded table: log_softmax(2 randn) per
context over the 194 tokens, the non-emittable columns at -30; weight 0.5) against the same plain beam decode with alpha_out, 26 steps,
alternating as --lexicon does; medians and spread over --repeats rounds, and their ratio.  With --general on the general kernels.
--nbest: after the decode timing of the first form, the read-out of its workspace: msocr_attn_beam_finalize + msocr_seq_confidence
(what every word pays today) and msocr_attn_beam_nbest for n_best 1, 3 and 8, each as the mean of 20 calls after 3 warm-up calls."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from manuscript_ocr_amd import _native as nat
from manuscript_ocr_amd import ops
from manuscript_ocr_amd.recognizers._trba import net
from manuscript_ocr_amd.recognizers._trba.net import AttnDecoder
from manuscript_ocr_amd import synth
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("B", nargs="?", type=int, default=1920)
ap.add_argument("--alpha", action="store_true")
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--general", action="store_true")
ap.add_argument("--greedy", action="store_true")
ap.add_argument("--nbest", action="store_true")
ap.add_argument("--forced", action="store_true")
ap.add_argument("--lexicon", type=int, default=0, metavar="N")
ap.add_argument("--lm", type=int, default=0, metavar="ORDER")
a = ap.parse_args()
if a.repeats < 1:
    ap.error("--repeats must be at least 1")
B, ALPHA, REPEATS = a.B, a.alpha, a.repeats
if a.general:
    net.HOIST_CTX = False
sd = synth.trba_state_dict(194, 256, seed=1)
decs = {"split": AttnDecoder(sd, 194, 256), "exact": AttnDecoder(sd, 194, 256, step_split=False)}  # precision "fp32" / "fp32-exact"
if a.general:
    decs = {"general": decs["exact"]}
torch.manual_seed(0)
bH = torch.randn(B, 13, 256, device="cuda")
pH = torch.randn(B, 13, 256, device="cuda")
if a.forced:
    import statistics
    name, dec = ("general", decs["general"]) if a.general else ("split", decs["split"])
    al = torch.empty((B, 26, 13), dtype=torch.float32, device="cuda")
    _lg, ids, _ = dec.greedy(bH, pH, 25, 1, 2, None, want_alpha=True, alpha_out=al)
    tok = torch.cat([torch.ones((B, 1), dtype=torch.int32, device="cuda"), ids[:, :-1]], 1).contiguous()
    variants = {"greedy + alpha": lambda: dec.greedy(bH, pH, 25, 1, 2, None, want_alpha=True, alpha_out=al),
                "forced": lambda: dec.forced(bH, pH, tok, 1, None)}
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _rep in range(REPEATS):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / 5)
            print(f"{name} {k}: {ms[k][-1]:.3f} ms per call (GEMM + kernel), B={B}, 26 steps")
    for k, v in ms.items():
        print(f"{name} {k}: median {statistics.median(v):.3f} ms, spread {max(v) - min(v):.3f} ms over {len(v)} rounds")
    sys.exit(0)
if a.lexicon:
    import statistics, time
    import numpy as np
    from manuscript_ocr_amd.recognizers import Lexicon
    name, dec = ("general", decs["general"]) if a.general else ("split", decs["split"])
    STEPS = 26
    itos = ["<PAD>", "<SOS>", "<EOS>"] + [chr(0x400 + i) for i in range(191)]
    rng = np.random.default_rng(a.lexicon)
    lens = np.clip(rng.poisson(8, size=a.lexicon), 1, STEPS - 1)
    t0 = time.perf_counter()
    lex = Lexicon(["".join(itos[i] for i in rng.integers(3, 194, size=n)) for n in lens], itos, STEPS)
    lex.to("cuda")
    print(f"lexicon: {len(lex)} words, {lex.n_nodes} nodes, root fan-out {int(lex.edge_begin[1])}, built and uploaded in {time.perf_counter() - t0:.2f} s")
    aws = torch.empty((B, STEPS, 8, 13), dtype=torch.float32, device="cuda")
    variants = {"beam + alpha": lambda: dec.beam(bH, pH, STEPS, 8, 0.9, 1.7, 1, 2, None, want_alpha=True, alpha_ws=aws),
                "lexicon": lambda: dec.beam(bH, pH, STEPS, 8, 0.9, 1.7, 1, 2, None, alpha_ws=aws, lexicon=lex)}
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _rep in range(REPEATS):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / 5)
            print(f"{name} {k}: {ms[k][-1]:.3f} ms per call (GEMM + kernel), B={B}, {STEPS} steps")
    for k, v in ms.items():
        print(f"{name} {k}: median {statistics.median(v):.3f} ms, spread {max(v) - min(v):.3f} ms over {len(v)} rounds")
    print(f"{name} lexicon / beam + alpha: {statistics.median(ms['lexicon']) / statistics.median(ms['beam + alpha']):.3f}")
    fin = variants["lexicon"]()[1]
    print(f"constrained finish steps: {int(fin.min())}..{int(fin.max())} (no chunk state: every launch runs all {STEPS} steps)")
    sys.exit(0)
if a.lm:
    import statistics
    from manuscript_ocr_amd.recognizers import CharLM
    name, dec = ("general", decs["general"]) if a.general else ("split", decs["split"])
    STEPS, V = 26, 194
    g = torch.Generator().manual_seed(a.lm)
    table = torch.log_softmax(2.0 * torch.randn(V ** (a.lm - 1), V, generator=g, dtype=torch.float64), -1)
    table[:, [0, 1]] = -30.0
    lm = CharLM(table.numpy(), V, a.lm, 1, 2)
    lm.to("cuda")
    print(f"language model: order {lm.order}, {lm.n_ctx} contexts x {V} tokens, {lm.table.nbytes / 1e6:.1f} MB on the device")
    aws = torch.empty((B, STEPS, 8, 13), dtype=torch.float32, device="cuda")
    variants = {"beam + alpha": lambda: dec.beam(bH, pH, STEPS, 8, 0.9, 1.7, 1, 2, None, want_alpha=True, alpha_ws=aws),
                "lm": lambda: dec.beam(bH, pH, STEPS, 8, 0.9, 1.7, 1, 2, None, alpha_ws=aws, lm=lm, lm_weight=0.5)}
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _rep in range(REPEATS):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / 5)
            print(f"{name} {k}: {ms[k][-1]:.3f} ms per call (GEMM + kernel), B={B}, {STEPS} steps")
    for k, v in ms.items():
        print(f"{name} {k}: median {statistics.median(v):.3f} ms, spread {max(v) - min(v):.3f} ms over {len(v)} rounds")
    print(f"{name} lm / beam + alpha: {statistics.median(ms['lm']) / statistics.median(ms['beam + alpha']):.3f}")
    fin = variants["lm"]()[1]
    print(f"fused finish steps: {int(fin.min())}..{int(fin.max())} (no chunk state: every launch runs all {STEPS} steps)")
    sys.exit(0)
if a.greedy:
    name, dec = ("general", decs["general"]) if a.general else ("split", decs["split"])
    al = torch.empty((B, 26, 13), dtype=torch.float32, device="cuda") if ALPHA else None
    gkw = {"want_alpha": True, "alpha_out": al} if ALPHA else {}
    for _ in range(2):
        dec.greedy(bH, pH, 25, 1, 2, None, **gkw)
    torch.cuda.synchronize()
    for _rep in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            dec.greedy(bH, pH, 25, 1, 2, None, **gkw)
        e1.record()
        torch.cuda.synchronize()
        print(f"{name} greedy: {e0.elapsed_time(e1) / 5:.3f} ms per call (GEMM + greedy kernel{' + alpha output' if ALPHA else ''}), B={B}")
    sys.exit(0)
def timed(fn, calls=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def time_nbest(dec, ws, B):
    """All 25 steps of every row (t_run = 25, as the decode above ran them): the read-out's largest case at this shape."""
    trun = torch.full((B,), 25, dtype=torch.int32, device="cuda")
    conf = torch.empty((B,), dtype=torch.float32, device="cuda")

    def today():
        lg, ids = dec.beam_finalize(ws, B, 25, 8, trun)
        nat.check(nat.lib().msocr_seq_confidence(lg.data_ptr(), ids.data_ptr(), trun.data_ptr(), B, dec.V, 25, conf.data_ptr(), ops._stream()),
                  "seq_confidence")

    base = timed(today)
    print(f"read-out, B={B}, V={dec.V}, K=8, 25 steps (ms per call, mean of 20):")
    print(f"  beam_finalize + seq_confidence: {base:.3f}")
    for n in (1, 3, 8):
        ms = timed(lambda: dec.beam_nbest(ws, B, 25, 8, trun, n, 2))
        print(f"  beam_nbest n_best={n}: {ms:.3f}  = {ms / base:.2f} x the pair above")


res = {}
aws = torch.empty((B, 25, 8, 13), dtype=torch.float32, device="cuda") if ALPHA else None
kw = {"want_alpha": True, "alpha_ws": aws} if ALPHA else {}
tag = " + alpha output" if ALPHA else ""
for mode, dec in decs.items():
    for _ in range(2):
        ws, fin, lp = dec.beam(bH, pH, 25, 8, 0.9, 1.7, 1, 2, None, **kw)[:3]
    torch.cuda.synchronize()
    for _rep in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            ws, fin, lp = dec.beam(bH, pH, 25, 8, 0.9, 1.7, 1, 2, None, **kw)[:3]
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 5
        print(f"{mode}: {ms:.3f} ms per call (GEMM + beam kernel{tag}), B={B}")
    trun = torch.full((B,), 25, dtype=torch.int32, device="cuda")
    logits, ids = dec.beam_finalize(ws, B, 25, 8, trun)
    res[mode] = (ms, logits.cpu(), ids.cpu())
    if a.nbest:
        time_nbest(dec, ws, B)
        sys.exit(0)
if a.general:
    sys.exit(0)
same = (res["split"][2] == res["exact"][2]).all(dim=1)
d = (res["split"][1] - res["exact"][1]).abs()
print(f"rows with identical ids: {int(same.sum())}/{B}; max |dlogit| on identical rows: {float(d[same].max()):.3e}")
for t in range(25):
    dt = d[:, t, :]
    print(f"step {t:2d}: max |dlogit| {float(dt.max()):.3e} (max |logit| {float(res['exact'][1][:, t].abs().max()):.2f}), rows > 1e-3: {int((dt.amax(dim=1) > 1e-3).sum())}")
