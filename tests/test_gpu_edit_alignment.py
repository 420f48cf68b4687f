"""msocr_edit_alignment on the MI355X against its host twin msocr_edit_alignment_host, which
tests/test_edit_alignment_cpu.py holds to the full table walked back by the four rules.  Distances, maps and counts are integers:
every comparison is equality, over all four output arrays.

Sizes straddle the kernels' own edges: 64 tokens = one block of the pattern = the rows of a traceback window, 4096 tokens = one
block per lane of the sweep (above it a lane owns two, above 8192 three, above 12288 four), text lengths around the 64 columns of a
window and the 64 steps a carry needs to cross the wave, and the cap of 16384 on both sides (64 MiB of trace).  The paths walk the
window refill: the pure diagonal through every window corner, a vertical run through several blocks in one column, a horizontal
run through several windows in one block."""
import numpy as np
import pytest

from test_edit_alignment_cpu import check_invariants, split
from test_edit_distance_long_cpu import CAP, csr, random_pair, structured_pairs

pytestmark = pytest.mark.gpu


def device_and_host(pairs):
    import torch
    from manuscript_ocr_amd import ops
    a_tok, a_off = csr([p[0] for p in pairs])
    b_tok, b_off = csr([p[1] for p in pairs])
    v = [p[2] for p in pairs]
    host = ops.edit_alignment_host(a_tok, a_off, b_tok, b_off, v)
    dev = ops.edit_alignment(torch.from_numpy(a_tok).cuda(), a_off, torch.from_numpy(b_tok).cuda(), b_off, v)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in dev], host


def assert_same(pairs):
    dev, host = device_and_host(pairs)
    for name, d, h in zip(("dist", "a_map", "b_map", "counts"), dev, host):
        assert d.dtype == h.dtype and d.shape == h.shape, name
        bad = np.flatnonzero((d != h).reshape(-1))
        assert bad.size == 0, (name, bad.size, bad[:8].tolist(), d.reshape(-1)[bad[:8]].tolist(), h.reshape(-1)[bad[:8]].tolist())
    return split(pairs, dev)


def edited(rng, a, v, n, foreign=1):
    """a text of n tokens that follows a: a's tokens (cycled) with a tenth replaced, so that every kind of step occurs"""
    b = np.resize(a, n).astype(np.int32) if len(a) and n else rng.integers(0, v + foreign, n).astype(np.int32)
    hit = rng.random(n) < 0.1
    b[hit] = rng.integers(0, v + foreign, int(hit.sum()))
    return b


def test_ragged_batch_with_empty_sides():
    rng = np.random.default_rng(21)
    lens = [(0, 0), (0, 40), (40, 0), (1, 1), (1, 300), (300, 1)] + [(int(m), int(n)) for m, n in rng.integers(0, 900, (27, 2))]
    assert len(lens) == 33
    pairs = []
    for k, (m, n) in enumerate(lens):
        v = (2, 4, 30, 1000)[k % 4]
        a = rng.integers(0, v, m).astype(np.int32)
        pairs.append((a, edited(rng, a, v, n, foreign=2), v))
    got = assert_same(pairs)
    assert [g[3] for g in got[:3]] == [[0, 0, 0, 0], [0, 0, 0, 40], [0, 0, 40, 0]]
    assert got[1][2] == [-1] * 40 and got[2][1] == [-1] * 40
    for pair, g in zip(pairs, got):
        check_invariants(pair, g)
    got = assert_same(structured_pairs())  # equal, disjoint, motif, garbage tokens, an empty alphabet
    assert got[0][3] == [1000, 0, 0, 0] and got[2][3] == [0, 1000, 0, 0] and got[10][3] == [0, 70, 60, 0]


@pytest.mark.parametrize("lens", [(63, 64, 65), (4095, 4096, 4097), (8192, 8193, 12288, 12289)], ids=lambda v: "-".join(map(str, v)))
def test_pattern_lengths_at_the_block_and_lane_edges(lens):
    rng = np.random.default_rng(lens[0])
    pairs = []
    for m in lens:
        for n, v in ((1, 4), (63, 30), (64, 2), (65, 4), (66, 30), (700, 30), (m + 1, 4)):
            a = rng.integers(0, v, m).astype(np.int32)
            pairs.append((a, edited(rng, a, v, n), v))
    assert_same(pairs)


def test_paths_that_stress_the_window_refill():
    rng = np.random.default_rng(71)
    same128, same4096 = rng.integers(0, 30, 128).astype(np.int32), rng.integers(0, 4, 4096).astype(np.int32)
    seq = rng.permutation(900).astype(np.int32)
    cut = np.concatenate([seq[:350], seq[550:]])                                        # 200 of the pattern's tokens removed
    put = np.concatenate([seq[:350], np.arange(2000, 2200, dtype=np.int32), seq[350:]])  # 200 foreign tokens put in
    pairs = [(same128, same128.copy(), 30), (same4096, same4096.copy(), 4), (seq, cut, 900), (seq, put, 900),
             (seq[:300], seq[300:600] + 0, 900), (seq[:130] % 7, seq[:700] % 7 + 7, 14)]
    got = assert_same(pairs)
    assert got[0][3] == [128, 0, 0, 0] and got[0][1] == list(range(128))               # the pure diagonal through every window corner
    assert got[1][3] == [4096, 0, 0, 0] and got[1][2] == list(range(4096))
    assert got[2][3] == [700, 0, 200, 0] and got[2][1][350:550] == [-1] * 200            # a vertical run through >= 3 blocks in one column
    assert got[2][1][:350] == list(range(350)) and got[2][1][550:] == list(range(350, 700))
    assert got[3][3] == [900, 0, 0, 200] and got[3][2][350:550] == [-1] * 200            # a horizontal run through >= 3 windows in one block
    assert got[4][3] == [0, 300, 0, 0] and got[5][3] == [0, 130, 0, 570]                # disjoint alphabets
    for pair, g in zip(pairs, got):
        check_invariants(pair, g)


def test_the_pair_at_the_cap_on_both_sides():
    rng = np.random.default_rng(31)
    a = rng.integers(0, 30, CAP).astype(np.int32)
    pair = (a, edited(rng, a, 30, CAP), 30)
    got = assert_same([pair])  # one pair, 64 MiB of trace
    check_invariants(pair, got[0])


def test_no_pairs_and_the_guards_behind_every_buffer():
    import torch
    from manuscript_ocr_amd import ops
    z = torch.zeros(0, dtype=torch.int32, device="cuda")
    none = ops.edit_alignment(z, [0], z, [0], [])
    assert [tuple(t.shape) for t in none] == [(0,), (0,), (0,), (0, 4)]
    rng = np.random.default_rng(51)
    pairs = [random_pair(rng, m, n, 30) for m, n in ((0, 5), (70, 0), (200, 129), (4097, 300), (64, 64), (65, 63))]
    a_tok, a_off = csr([p[0] for p in pairs])
    b_tok, b_off = csr([p[1] for p in pairs])
    v = [p[2] for p in pairs]
    N, na, nb = len(pairs), len(a_tok), len(b_tok)
    bufs = [torch.full((k + 64,), -7, dtype=torch.int32, device="cuda") for k in (N, na, nb, 4 * N)]
    need = ops.edit_alignment_workspace_bytes(a_off, b_off, v)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")  # exactly the stated sizes are handed over; the rest is a guard
    out = (bufs[0][:N], bufs[1][:na], bufs[2][:nb], bufs[3][:4 * N].view(N, 4))
    ops.edit_alignment(torch.from_numpy(a_tok).cuda(), a_off, torch.from_numpy(b_tok).cuda(), b_off, v, workspace=ws[:need], out=out)
    torch.cuda.synchronize()
    for got, want in zip(out, ops.edit_alignment_host(a_tok, a_off, b_tok, b_off, v)):
        assert got.cpu().numpy().tolist() == want.tolist()
    for buf, k in zip(bufs, (N, na, nb, 4 * N)):
        assert bool((buf[k:] == -7).all())
    assert bool((ws[need:] == 0xA5).all())


@pytest.mark.parametrize("shift", [0, 3])
def test_first_offsets_above_zero_and_views(shift):
    """The first test on the device with a_off[0] > 0 and b_off[0] > 0: a_base / b_base of eal_traceback_kernel are not 0, and
    p.a0 / p.b0 of the mask and sweep kernels count from inside the token arrays, which carry junk before the first offset and
    behind the last.  The maps hold a_off[N] - a_off[0] and b_off[N] - b_off[0] entries and begin at the first pair's tokens: a map
    written at its array index instead lands in the guard.  shift = 3: the token arrays are the views buf[3:] of a fresh allocation
    besides.  Guards of -7 on both sides of every output; the host twin gets the same arrays and offsets."""
    import torch
    from manuscript_ocr_amd import ops
    rng = np.random.default_rng(52)
    pairs = [random_pair(rng, m, n, 30) for m, n in ((0, 5), (70, 0), (200, 129), (4097, 300), (64, 64), (65, 63))]
    a_tok, a_off = csr([p[0] for p in pairs])
    b_tok, b_off = csr([p[1] for p in pairs])
    v = [p[2] for p in pairs]
    clean = ops.edit_alignment_host(a_tok, a_off, b_tok, b_off, v)
    # the junk repeats the neighbouring tokens, so that a table or a sweep that starts early or ends late finds matches there
    a_tok, a_off = np.concatenate([a_tok[:37], a_tok, a_tok[-21:]]), a_off + 37
    b_tok, b_off = np.concatenate([b_tok[:5], b_tok, b_tok[-66:]]), b_off + 5
    N, na, nb = len(pairs), int(a_off[-1] - a_off[0]), int(b_off[-1] - b_off[0])
    assert a_off[0] == 37 and b_off[0] == 5 and na == len(a_tok) - 58 and nb == len(b_tok) - 71
    want = ops.edit_alignment_host(a_tok, a_off, b_tok, b_off, v)
    for w, c in zip(want, clean):
        assert w.shape == c.shape and w.tolist() == c.tolist()    # the host twin reads nothing outside the offsets
    views = []
    for tok in (a_tok, b_tok):
        buf = torch.full((shift + len(tok),), -3, dtype=torch.int32, device="cuda")
        buf[shift:] = torch.from_numpy(tok).cuda()
        views.append(buf[shift:])
        assert views[-1].data_ptr() % 16 == 4 * shift
    G = 64
    sizes = (N, na, nb, 4 * N)
    bufs = [torch.full((G + k + G,), -7, dtype=torch.int32, device="cuda") for k in sizes]
    out = (bufs[0][G:G + N], bufs[1][G:G + na], bufs[2][G:G + nb], bufs[3][G:G + 4 * N].view(N, 4))
    ops.edit_alignment(views[0], a_off, views[1], b_off, v, out=out)
    torch.cuda.synchronize()
    for name, got, w in zip(("dist", "a_map", "b_map", "counts"), out, want):
        assert got.cpu().numpy().tolist() == w.tolist(), name
    for buf, k in zip(bufs, sizes):
        assert bool((buf[:G] == -7).all()) and bool((buf[G + k:] == -7).all())
    # without `out` the maps have the length of the offsets' span, not of the token arrays
    fresh = ops.edit_alignment(views[0], a_off, views[1], b_off, v)
    assert [tuple(t.shape) for t in fresh] == [(N,), (na,), (nb,), (N, 4)]
    for got, w in zip(fresh, want):
        assert got.cpu().numpy().tolist() == w.tolist()
    for pair, g in zip(pairs, split(pairs, [t.cpu().numpy() for t in fresh])):
        check_invariants(pair, g)


def same_alignments(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert tuple(x[:5]) == tuple(y[:5])
        assert x.ref_to_hyp.tolist() == y.ref_to_hyp.tolist() and x.hyp_to_ref.tolist() == y.hyp_to_ref.tolist()


def test_sequence_alignments_and_the_breakdown_on_the_device():
    from manuscript_ocr_amd.recognizers import error_breakdown, sequence_alignments, text_error_rates
    rng = np.random.default_rng(61)
    vocab = [f"w{k}" for k in range(400)]
    refs, hyps = [], []
    for k in range(6):
        words = [vocab[int(i)] for i in rng.integers(0, 400, 300 + 50 * k)]
        hyp = list(words)
        for _ in range(20):
            hyp[int(rng.integers(0, len(hyp)))] = "??"
        del hyp[40:40 + 7 * k]
        hyp[100:100] = ["new"] * k
        refs.append(" ".join(words))
        hyps.append(" ".join(hyp))
    seq_r = refs + [r.split() for r in refs] + ["", "abc", []]
    seq_h = hyps + [h.split() for h in hyps] + ["xy", "", ["only"]]
    on_host = sequence_alignments(seq_r, seq_h)
    same_alignments(sequence_alignments(seq_r, seq_h, device="cuda"), on_host)
    assert [a.distance for a in on_host[-3:]] == [2, 3, 1]
    assert error_breakdown(seq_r, seq_h, device="cuda") == error_breakdown(seq_r, seq_h)
    a, b = text_error_rates(refs, hyps, device="cuda", breakdown=True), text_error_rates(refs, hyps, breakdown=True)
    plain = text_error_rates(refs, hyps)
    assert set(a) == set(b)
    for key in b:
        if key == "word_alignments":
            same_alignments(a[key], b[key])
        elif isinstance(b[key], np.ndarray):
            assert a[key].tolist() == b[key].tolist(), key
        else:
            assert a[key] == b[key], key
    for key in plain:
        assert (a[key].tolist() == plain[key].tolist()) if isinstance(plain[key], np.ndarray) else (a[key] == plain[key]), key
    assert a["word_counts"][:, 3].tolist() == list(range(6)) and 0 < a["wer_micro"] < 1


def test_pipeline_transfer_text_with_the_package_plugins():
    """Pipeline.transfer_text with EAST + TRBA on a synthetic page: against the pipeline's own text every word is paired at
    distance 0; with one word removed from the transcription and one altered, exactly one word stays alone and one is paired at a
    distance above 0.  The device route and the host twin agree word for word."""
    from manuscript_ocr_amd import Pipeline, synth
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.detectors._types import TransferWord
    from manuscript_ocr_amd.recognizers import TRBA
    H, W = 512, 768
    det = EAST(state_dict=synth.east_state_dict(), target_size=(W, H), device="cuda")
    rec = TRBA(state_dict=synth.trba_state_dict(194, 256, seed=20260128), config={"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256},
               device="cuda")
    pipe = Pipeline(detector=det, recognizer=rec)
    img = synth.synth_page(5, H, W)[0]
    own = [w.text for b in pipe.predict(img).blocks for w in b.words if w.text]
    assert len(own) >= 2

    def both(gt):
        res = []
        for device in (rec.device, None):
            page, unpaired = pipe.transfer_text(img, gt, device=device)
            words = [w for b in page.blocks for w in b.words if w.text]
            assert [w.text for w in words] == own and all(type(w) is TransferWord for w in words)
            res.append(([(w.gt_text, w.gt_index, w.char_distance) for w in words], unpaired))
        assert res[0] == res[1]
        return res[0]

    rows, unpaired = both(" ".join(own))
    assert rows == [(t, k, 0) for k, t in enumerate(own)] and unpaired == []
    # one word removed from the transcription, one altered by a character no recognised word ends with
    gone, changed = 0, len(own) - 1
    gt = [t for k, t in enumerate(own) if k != gone]
    gt[-1] = own[changed] + "†"
    rows, unpaired = both(" ".join(gt))
    assert sum(1 for r in rows if r[0] is None) == 1 and sum(1 for r in rows if r[2] is not None and r[2] > 0) == 1
    assert rows[gone] == (None, None, None) and rows[changed] == (gt[-1], len(gt) - 1, 1) and unpaired == []
