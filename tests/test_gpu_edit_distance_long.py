"""msocr_edit_distance_long on the MI355X against its host twin msocr_edit_distance_long_host, which
tests/test_edit_distance_long_cpu.py holds to a plain row programme.  Distances are integers: every comparison is equality.

Sizes straddle the kernel's own edges: 64 tokens = one block of the pattern, 4096 tokens = 64 blocks = one block per lane of the wave
(above it a lane owns two, above 8192 three, above 12288 four), text lengths around the 64 steps a carry needs to cross the wave, and
the cap of 16384 on both sides."""
import numpy as np
import pytest

from test_edit_distance_long_cpu import CAP, csr, random_pair, structured_pairs

pytestmark = pytest.mark.gpu


def device_and_host(pairs):
    import torch
    from manuscript_ocr_amd import ops
    a_tok, a_off = csr([p[0] for p in pairs])
    b_tok, b_off = csr([p[1] for p in pairs])
    v = [p[2] for p in pairs]
    host = ops.edit_distance_long_host(a_tok, a_off, b_tok, b_off, v)
    dev = ops.edit_distance_long(torch.from_numpy(a_tok).cuda(), a_off, torch.from_numpy(b_tok).cuda(), b_off, v)
    torch.cuda.synchronize()
    return dev.cpu().numpy().tolist(), host.tolist()


def edited(rng, a, v, n, foreign=1):
    """a text of n tokens that follows a: a's tokens (cycled) with a tenth replaced, so that the distance is neither 0 nor max"""
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
    dev, host = device_and_host(pairs)
    assert dev == host
    assert dev[:3] == [0, 40, 40]
    dev, host = device_and_host(structured_pairs())  # equal, disjoint, motif, garbage tokens, an empty alphabet
    assert dev == host and dev[0] == 0 and dev[2] == 1000


@pytest.mark.parametrize("lens", [(63, 64, 65), (4095, 4096, 4097), (8192, 8193, 12288, 12289)], ids=lambda v: "-".join(map(str, v)))
def test_pattern_lengths_at_the_block_and_lane_edges(lens):
    rng = np.random.default_rng(lens[0])
    pairs = []
    for m in lens:
        for n, v in ((1, 4), (63, 30), (64, 2), (65, 4), (700, 30), (m, 4), (m + 1, 30)):
            a = rng.integers(0, v, m).astype(np.int32)
            pairs.append((a, edited(rng, a, v, n), v))
    dev, host = device_and_host(pairs)
    assert dev == host


def test_pattern_at_the_cap():
    rng = np.random.default_rng(31)
    a = rng.integers(0, 30, CAP).astype(np.int32)
    pairs = [(a, edited(rng, a, 30, n), 30) for n in (1, 62, 63, 64, 65, 66, 5000)]
    pairs.append((a[:CAP - 1], edited(rng, a, 30, 5000), 30))
    dev, host = device_and_host(pairs)
    assert dev == host


def test_alphabets_of_one_and_of_the_cap():
    """v = 1: one table row that every matching token reads.  v = 16384 with 16384 distinct pattern tokens: the word case at the cap,
    a table of 16384 x 256 words with one bit per row."""
    rng = np.random.default_rng(41)
    ones = np.zeros(5000, dtype=np.int32)
    mixed = (rng.random(4000) < 0.3).astype(np.int32)  # 0 matches, 1 equals nothing
    distinct = rng.permutation(CAP).astype(np.int32)
    moved = np.concatenate([distinct[9000:12000], distinct[:9000], distinct[12000:]])
    moved[::97] = CAP + 5
    pairs = [(ones, mixed, 1), (ones[:64], ones[:65], 1), (distinct, moved, CAP), (distinct, distinct[::-1].copy(), CAP)]
    dev, host = device_and_host(pairs)
    assert dev == host
    assert dev[1] == 1 and dev[0] == 5000 - int((mixed == 0).sum())


def test_no_pairs_and_the_guard_behind_the_distances():
    import torch
    from manuscript_ocr_amd import ops
    none = ops.edit_distance_long(torch.zeros(0, dtype=torch.int32, device="cuda"), [0], torch.zeros(0, dtype=torch.int32, device="cuda"),
                                  [0], [])
    assert none.shape == (0,)
    rng = np.random.default_rng(51)
    pairs = [random_pair(rng, m, n, 30) for m, n in ((0, 5), (70, 0), (200, 129), (4097, 300), (64, 64))]
    a_tok, a_off = csr([p[0] for p in pairs])
    b_tok, b_off = csr([p[1] for p in pairs])
    v = [p[2] for p in pairs]
    N = len(pairs)
    buf = torch.full((N + 64,), -7, dtype=torch.int32, device="cuda")
    need = ops.edit_distance_long_workspace_bytes(a_off, b_off, v)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")  # exactly the stated size is handed over; the rest is a guard
    ops.edit_distance_long(torch.from_numpy(a_tok).cuda(), a_off, torch.from_numpy(b_tok).cuda(), b_off, v, workspace=ws[:need], out=buf[:N])
    torch.cuda.synchronize()
    assert buf[:N].cpu().numpy().tolist() == ops.edit_distance_long_host(a_tok, a_off, b_tok, b_off, v).tolist()
    assert bool((buf[N:] == -7).all()) and bool((ws[need:] == 0xA5).all())


@pytest.mark.parametrize("shift", [0, 3])
def test_first_offsets_above_zero_and_views(shift):
    """The first test on the device with a_off[0] > 0 and b_off[0] > 0: p.a0 / p.b0 of the mask and sweep kernels count from inside
    the token arrays, which carry junk before the first offset and behind the last (the neighbouring tokens again, so that a table
    or a sweep that starts early or ends late finds matches there).  shift = 3: the token arrays are the views buf[3:] of a fresh
    allocation besides.  A guard of -7 on both sides of the distances; the host twin gets the same arrays and offsets."""
    import torch
    from manuscript_ocr_amd import ops
    rng = np.random.default_rng(52)
    pairs = [random_pair(rng, m, n, 30) for m, n in ((0, 5), (70, 0), (200, 129), (4097, 300), (64, 64), (65, 63))]
    a_tok, a_off = csr([p[0] for p in pairs])
    b_tok, b_off = csr([p[1] for p in pairs])
    v = [p[2] for p in pairs]
    clean = ops.edit_distance_long_host(a_tok, a_off, b_tok, b_off, v)
    a_tok, a_off = np.concatenate([a_tok[:37], a_tok, a_tok[-21:]]), a_off + 37
    b_tok, b_off = np.concatenate([b_tok[:5], b_tok, b_tok[-66:]]), b_off + 5
    assert a_off[0] == 37 and b_off[0] == 5 and a_off[-1] == len(a_tok) - 21 and b_off[-1] == len(b_tok) - 66
    want = ops.edit_distance_long_host(a_tok, a_off, b_tok, b_off, v)
    assert want.tolist() == clean.tolist()                        # the host twin reads nothing outside the offsets
    views = []
    for tok in (a_tok, b_tok):
        buf = torch.full((shift + len(tok),), -3, dtype=torch.int32, device="cuda")
        buf[shift:] = torch.from_numpy(tok).cuda()
        views.append(buf[shift:])
        assert views[-1].data_ptr() % 16 == 4 * shift
    N, G = len(pairs), 64
    buf = torch.full((G + N + G,), -7, dtype=torch.int32, device="cuda")
    ops.edit_distance_long(views[0], a_off, views[1], b_off, v, out=buf[G:G + N])
    torch.cuda.synchronize()
    assert buf[G:G + N].cpu().numpy().tolist() == want.tolist()
    assert bool((buf[:G] == -7).all()) and bool((buf[G + N:] == -7).all())
    assert ops.edit_distance_long(views[0], a_off, views[1], b_off, v).cpu().numpy().tolist() == want.tolist()


def test_sequence_edit_distances_on_the_device():
    from manuscript_ocr_amd.recognizers import sequence_edit_distances, text_error_rates
    rng = np.random.default_rng(61)
    vocab = [f"w{k}" for k in range(400)]
    refs, hyps = [], []
    for k in range(6):
        words = [vocab[int(i)] for i in rng.integers(0, 400, 300 + 50 * k)]
        hyp = list(words)
        for _ in range(20):
            hyp[int(rng.integers(0, len(hyp)))] = "??"
        del hyp[40:40 + 7 * k]
        refs.append(" ".join(words))
        hyps.append(" ".join(hyp))
    seq_r = refs + [r.split() for r in refs] + ["", "abc", []]
    seq_h = hyps + [h.split() for h in hyps] + ["xy", "", ["only"]]
    on_host = sequence_edit_distances(seq_r, seq_h)
    assert sequence_edit_distances(seq_r, seq_h, device="cuda").tolist() == on_host.tolist()
    assert on_host[-3:].tolist() == [2, 3, 1]
    a, b = text_error_rates(refs, hyps, device="cuda"), text_error_rates(refs, hyps)
    for key in ("char_dist", "word_dist", "bag_errors", "ref_chars", "ref_words", "cer", "wer"):
        assert a[key].tolist() == b[key].tolist(), key
    assert a["cer_micro"] == b["cer_micro"] and a["wer_micro"] == b["wer_micro"] and 0 < a["wer_micro"] < 1


def test_pipeline_evaluate_text_with_the_package_plugins():
    """Pipeline.evaluate_text on the device route (TRBA's device for the distances) gives the host twin's figures: zeros against the
    pipeline's own text; against its words reversed the bag stays whole and the order costs word errors."""
    from manuscript_ocr_amd import Pipeline, synth
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.recognizers import TRBA, text_error_rates
    H, W = 512, 768
    det = EAST(state_dict=synth.east_state_dict(), target_size=(W, H), device="cuda")
    rec = TRBA(state_dict=synth.trba_state_dict(194, 256, seed=20260128), config={"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256},
               device="cuda")
    pipe = Pipeline(detector=det, recognizer=rec)
    img = synth.synth_page(5, H, W)[0]
    own = " ".join(w.text for b in pipe.predict(img).blocks for w in b.words if w.text)
    assert len(own.split()) >= 2
    gts = [own, " ".join(reversed(own.split()))]
    r = pipe.evaluate_text([img, img], gts)
    assert r["hypotheses"] == [own, own]
    want = text_error_rates(gts, r["hypotheses"])  # the host twin
    for key in ("char_dist", "word_dist", "bag_errors", "ref_chars", "ref_words", "cer", "wer"):
        assert r[key].tolist() == want[key].tolist(), key
    for key in ("n", "cer_micro", "wer_micro", "cer_mean", "wer_mean", "bag_error_rate"):
        assert r[key] == want[key], key
    assert r["char_dist"][0] == 0 and r["word_dist"][0] == 0 and r["bag_errors"].tolist() == [0, 0]
    if gts[1] != " ".join(own.split()):  # unless the page reads the same backwards
        assert r["word_dist"][1] > 0 and r["wer_micro"] > 0
