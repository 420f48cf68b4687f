"""Times the confusion-weighted nearest-word lookup (msocr_lexicon_nearest_weighted) beside the unit-cost lookup
on the same inputs, the weighted host twin on a subset of the rows, and the transfers (dev tool).
  python tools/lexicon_nearest_weighted_time.py [--repeats N] [--k K] [--host-rows R]
The shapes of tools/nearest_time.py: B = 1920 and 7680 rows (7680 = the words of one bench step) of 25 steps and lexicons of 1 000 and
100 000 seeded random words (lengths 1..24, mean about 8, over the 191 symbols), k = 3, without a bound and with a bound of two unit
edits (max_distance 2 for the unit-cost kernel, 2 * 32 cost units for the weighted one).  Half of the rows are lexicon words with 0..2
random substitutions, half are independent draws.  The costs are EditCosts.from_confusions' scale (1..32, unknown 32) with seeded
random entries, a tenth of the substitutions cheap.  Per round 3 calls of every variant in turn; one line per variant with the median
and the spread (max - min) over --repeats rounds (default 5), and the ratio weighted / unit-cost.  The host twin runs once over the
first --host-rows rows (default 16; one core) and is reported per row and scaled to B.  Transfers: the cost tables to the device
(once per EditCosts and device), the ids of B rows to the device and the k results back.  The device results are compared with the
host twin on the timed subset."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from manuscript_ocr_amd.recognizers import EditCosts, Lexicon
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--k", type=int, default=3)
ap.add_argument("--host-rows", type=int, default=16)
a = ap.parse_args()
STEPS, K, UNIT, CALLS = 25, a.k, 32, 3
itos = ["<PAD>", "<SOS>", "<EOS>"] + [chr(0x400 + i) for i in range(191)]
V = len(itos)


def make_costs():
    rng = np.random.default_rng(5)
    sub = np.where(rng.random((V, V)) < 0.1, rng.integers(1, 12, (V, V)), rng.integers(20, UNIT + 1, (V, V)))
    np.fill_diagonal(sub, 0)
    return EditCosts(sub, rng.integers(8, UNIT + 1, V), rng.integers(8, UNIT + 1, V), itos, unknown=UNIT)


def make_lexicon(n):
    rng = np.random.default_rng(n)
    lens = np.clip(rng.poisson(8, size=n), 1, STEPS - 1)
    lex = Lexicon(["".join(itos[i] for i in rng.integers(3, 194, size=m)) for m in lens], itos, STEPS)
    lex.wordlist("cuda")
    print(f"lexicon: {len(lex)} words, {len(lex.word_tok)} tokens")
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


def event_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


costs = make_costs()
torch.cuda.synchronize()
t0 = time.perf_counter()
costs.to("cuda")
torch.cuda.synchronize()
print(f"cost tables ({costs.sub.nbytes + costs.delete.nbytes + costs.insert.nbytes} bytes) to the device, first use: "
      f"{(time.perf_counter() - t0) * 1e3:.3f} ms")
variants, host = {}, {}
for n in (1000, 100000):
    lex = make_lexicon(n)
    for B in (1920, 7680):
        ids = make_rows(lex, B, B + n)
        ids_dev = torch.from_numpy(ids).cuda()
        trun_dev = torch.full((B,), STEPS, dtype=torch.int32, device="cuda")
        pinned = torch.from_numpy(ids).pin_memory()
        variants[f"ids of B {B} to the device ({ids.nbytes} bytes, pinned)"] = lambda p=pinned: p.to("cuda", non_blocking=True)
        for bound_units in (None, 2):
            wb = None if bound_units is None else bound_units * UNIT
            R = min(a.host_rows, B)
            t0 = time.perf_counter()
            want = lex.nearest(ids[:R], None, K, wb, costs=costs)
            host_ms = (time.perf_counter() - t0) * 1e3 / R
            got = [t.cpu().numpy() for t in lex.nearest_device(ids_dev[:R], trun_dev[:R], K, wb, costs)]
            assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
            idx = lex.nearest_device(ids_dev, trun_dev, K, wb, costs)[0]
            filled = float((idx[:, 0] >= 0).float().mean())
            what = f"B {B}, {n} words, k {K}, " + ("no bound" if bound_units is None else f"bound {bound_units} units")
            print(f"{what}: rows with a weighted suggestion {filled:.3f}")
            host[what] = (host_ms, R)
            variants["weighted, " + what] = (lambda lex=lex, i=ids_dev, t=trun_dev, bd=wb: lex.nearest_device(i, t, K, bd, costs))
            variants["unit-cost, " + what] = (lambda lex=lex, i=ids_dev, t=trun_dev, bd=bound_units: lex.nearest_device(i, t, K, bd))
        out = lex.nearest_device(ids_dev, trun_dev, K, None, costs)
        variants[f"results of B {B} to the host (2 x {out[0].numel() * 4} bytes, {n} words)"] = lambda o=out: (o[0].cpu(), o[1].cpu())
for fn in variants.values():
    fn()
torch.cuda.synchronize()
ms = {k: [] for k in variants}
for _rep in range(a.repeats):
    for k, fn in variants.items():
        ms[k].append(event_ms(fn, CALLS))
med = {k: statistics.median(v) for k, v in ms.items()}
for k, v in ms.items():
    print(f"{k}: median {med[k]:.3f} ms, spread {max(v) - min(v):.3f} ms over {len(v)} rounds")
print("ratios:")
for what, (host_ms, R) in host.items():
    B = int(what.split()[1].rstrip(","))
    w, u = med["weighted, " + what], med["unit-cost, " + what]
    print(f"{what}: weighted / unit-cost {w / u:.1f} x; host twin {host_ms:.3f} ms per row over {R} rows on one core = "
          f"{host_ms * B:.0f} ms for B rows, {host_ms * B / w:.0f} x the device")
