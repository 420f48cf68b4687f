"""Times the beam-8 decode launch (all 25 steps, no early exit) for B crops, split-operand form against exact-f32 MFMA (dev tool).
  python tools/attn_time.py [B] [--alpha] [--repeats N] [--general] [--greedy]
--alpha: with the attention-weight output on (the _alpha entry points, into one preallocated buffer).  --repeats N: N timed repeats
of 5 calls each per form, one line each (default 1).  --general: the general kernel (csrc/attn_general.hip) at the same shape
instead of the matrix-core kernels (net.HOIST_CTX = False; one form, no split / exact comparison).  --greedy: the greedy decode
(26 steps) instead of the beam decode: the matrix-core greedy kernel, or the general one with --general; timings only."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from manuscript_ocr_amd.recognizers._trba import net
from manuscript_ocr_amd.recognizers._trba.net import AttnDecoder
from manuscript_ocr_amd import synth
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("B", nargs="?", type=int, default=1920)
ap.add_argument("--alpha", action="store_true")
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--general", action="store_true")
ap.add_argument("--greedy", action="store_true")
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
if a.general:
    sys.exit(0)
same = (res["split"][2] == res["exact"][2]).all(dim=1)
d = (res["split"][1] - res["exact"][1]).abs()
print(f"rows with identical ids: {int(same.sum())}/{B}; max |dlogit| on identical rows: {float(d[same].max()):.3e}")
for t in range(25):
    dt = d[:, t, :]
    print(f"step {t:2d}: max |dlogit| {float(dt.max()):.3e} (max |logit| {float(res['exact'][1][:, t].abs().max()):.2f}), rows > 1e-3: {int((dt.amax(dim=1) > 1e-3).sum())}")
