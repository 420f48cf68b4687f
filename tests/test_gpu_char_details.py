"""Per-symbol confidence and position through the public interface: TRBA.predict(return_chars=True), the recognize_start /
recognize_finish pair with char_details, and Pipeline with `char_details = True`.  Synthetic weights, 32 x 100 canvases, greedy and
beam.  The values' arithmetic is checked in test_gpu_attn_alpha.py; here: that the feature changes nothing else, that the symbols
line up with the text, that positions stay inside their window, and that the flag is off unless asked for."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = {"img_h": 32, "img_w": 100, "max_len": 25, "hidden_size": 256}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def rec(gpu):
    from manuscript_ocr_amd import synth
    from manuscript_ocr_amd.recognizers import TRBA
    return TRBA(state_dict=synth.trba_state_dict_confident(194, 256, seed=3), config=CFG, device="cuda")


@pytest.fixture(scope="module")
def crops():
    """40 crops of 32 x 100, every third cut to 32 x 60 (its resized copy fills 60 of the canvas's 100 columns: padding) and every
    fifth to 20 x 100 (resized to 100 columns, 20 rows)."""
    from manuscript_ocr_amd import synth
    out = []
    for k, c in enumerate(synth.synth_crops(1, 40, 32, 100)):
        out.append(np.ascontiguousarray(c[:, :60] if k % 3 == 1 else c[:20] if k % 5 == 2 else c))
    return out


@pytest.mark.parametrize("mode", ["greedy", "beam"])
def test_predict_return_chars(rec, crops, mode):
    plain = rec.predict(crops, mode=mode)
    detailed = rec.predict(crops, mode=mode, return_chars=True)
    assert len(plain) == len(detailed) == 40
    assert all(set(p) == {"text", "confidence"} for p in plain), "off by default: the reference's result dicts"
    n_chars = 0
    for crop, p, d in zip(crops, plain, detailed):
        assert d["text"] == p["text"] and d["confidence"] == p["confidence"]
        assert set(d) == {"text", "confidence", "chars"}
        assert "".join(c["char"] for c in d["chars"]) == d["text"]
        src_w = crop.shape[1]
        for c in d["chars"]:
            assert set(c) == {"char", "confidence", "x"}
            assert 0.0 <= c["confidence"] <= 1.0
            assert 0.0 <= c["x"] <= src_w, (c["x"], src_w)
        n_chars += len(d["chars"])
    assert n_chars > 100, "the planted decoder writes words"


@pytest.mark.parametrize("mode", ["greedy", "beam"])
def test_recognize_finish_char_details(rec, crops, mode):
    canv = torch.from_numpy(rec._canvases(crops)).cuda()
    spans = [(0, 25), (25, 15)]  # two pages: chunks of 25 and 15 rows with run lengths of their own
    plain = rec.recognize_finish(rec.recognize_start(canv, mode, spans=spans), spans=spans)
    out = rec.recognize_finish(rec.recognize_start(canv, mode, spans=spans, char_details=True), spans=spans)
    assert len(plain) == 3 and len(out) == 6
    ids, trun, conf, prob, centre, peak = out
    for a, b in zip(plain, out[:3]):
        assert np.array_equal(a, b)
    steps = rec.max_length + 1 if mode == "greedy" else rec.max_length
    assert prob.shape == centre.shape == peak.shape == (40, steps)
    assert prob.dtype == np.float32 and centre.dtype == np.float32 and peak.dtype == np.int32
    T = 13  # 100 columns / 8 + 1
    for b in range(40):
        t = int(trun[b])
        assert t >= 1
        assert abs(float(prob[b, :t].astype(np.float64).mean()) - float(conf[b])) <= 64 * 2.0 ** -24, b
        assert (prob[b, t:] == 0).all() and (centre[b, t:] == 0).all() and (peak[b, t:] == -1).all()
        assert ((peak[b, :t] >= 0) & (peak[b, :t] < T)).all()
        # a convex combination of the frame centres 0.5 .. T - 0.5, up to the row sum's rounding (64 * 2^-24, times at most T)
        assert ((centre[b, :t] >= 0.5 - 1e-4) & (centre[b, :t] <= T - 0.5 + 1e-4)).all()
    # with logits as well: they come before the details
    full = rec.recognize_finish(rec.recognize_start(canv, mode, spans=spans, char_details=True), spans=spans, return_logits=True)
    assert len(full) == 7 and full[3].shape == (40, steps, 194) and np.array_equal(full[4], prob) and np.array_equal(full[6], peak)


def _pages_and_maps():
    from manuscript_ocr_amd import synth
    H, W = 224, 320
    pages, maps = [], []
    for seed in (41, 42):
        pg, rects = synth.synth_page(seed, H, W)
        pages.append(pg)
        maps.append(synth.synth_maps(rects, (H, W), (H // 4, W // 4), seed))
    mo = (torch.from_numpy(np.stack([m[0] for m in maps])).cuda(), torch.from_numpy(np.stack([m[1] for m in maps])).cuda())
    return pages, mo


def test_pipeline_char_details(gpu, rec):
    from manuscript_ocr_amd import Pipeline, synth
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.detectors._types import CharWord, Word
    H, W = 224, 320
    pipe = Pipeline(EAST(state_dict=synth.east_state_dict(), target_size=(W, H), device="cuda"), rec)
    pages, mo = _pages_and_maps()
    assert not getattr(pipe, "char_details", False)
    off = pipe.predict_batch(pages, _maps_override=mo)
    assert not any(isinstance(w, CharWord) for p in off for w in p.blocks[0].words)
    key = lambda p: [(w.polygon, w.detection_confidence, w.text, w.recognition_confidence) for w in p.blocks[0].words]
    pipe.char_details = True
    for device_order in (True, False):  # crops ordered and described on the device, and the host path
        pipe.device_order = device_order
        on = pipe.predict_batch(pages, _maps_override=mo)
        n_words = 0
        for p_on, p_off in zip(on, off):
            assert key(p_on) == key(p_off)
            assert p_on.model_dump() == p_off.model_dump()
            for w in p_on.blocks[0].words:
                if w.text is None:
                    assert type(w) is Word  # too small to recognise: left as it was
                    continue
                assert isinstance(w, CharWord)
                assert "".join(c.char for c in w.chars) == w.text
                xs = [pt[0] for pt in np.array(w.polygon, dtype=np.int32).tolist()]
                x1, x2 = max(0, min(xs)), min(W, max(xs))  # the clamped AABB the crop was cut from
                assert all(x1 <= c.x <= x2 for c in w.chars), (x1, x2, [c.x for c in w.chars])
                assert all(0.0 <= c.confidence <= 1.0 for c in w.chars)
                n_words += 1
        assert n_words == sum(w.text is not None for p in off for w in p.blocks[0].words) > 0, n_words
    pipe.char_details = False
    again = pipe.predict_batch(pages, _maps_override=mo)
    assert [key(p) for p in again] == [key(p) for p in off]
    assert not any(isinstance(w, CharWord) for p in again for w in p.blocks[0].words)


def test_graph_path_is_kept_without_details_and_declined_with(gpu, monkeypatch):
    """use_graphs=True: with the flag off the second call of a bucket replays a captured graph (handle.graph_inst); with it on
    recognize_start_graph declines and the eager path returns the same words."""
    from manuscript_ocr_amd import Pipeline, synth
    from manuscript_ocr_amd.detectors import EAST
    from manuscript_ocr_amd.detectors._types import CharWord
    from manuscript_ocr_amd.recognizers import TRBA
    H, W = 224, 320
    grec = TRBA(state_dict=synth.trba_state_dict_confident(194, 256, seed=3), config=CFG, device="cuda", use_graphs=True)
    pipe = Pipeline(EAST(state_dict=synth.east_state_dict(), target_size=(W, H), device="cuda"), grec)
    pipe.stream_sets = 1  # one set of launch streams: consecutive calls land in the same graph bucket
    pages, mo = _pages_and_maps()
    pages_dev = torch.from_numpy(np.stack(pages)).cuda()  # graphs are keyed by the page tensor
    seen = []
    finish = grec.recognize_finish

    def spy(handle, *a, **kw):
        seen.append((handle.graph_inst is not None, bool(handle.char_details)))
        return finish(handle, *a, **kw)

    monkeypatch.setattr(grec, "recognize_finish", spy)
    key = lambda p: [(w.polygon, w.detection_confidence, w.text, w.recognition_confidence) for w in p.blocks[0].words]
    first = pipe.predict_batch(pages, pages_dev=pages_dev, _maps_override=mo)
    second = pipe.predict_batch(pages, pages_dev=pages_dev, _maps_override=mo)
    assert seen == [(False, False), (True, False)], seen
    assert [key(p) for p in first] == [key(p) for p in second]
    assert not any(isinstance(w, CharWord) for p in second for w in p.blocks[0].words)
    pipe.char_details = True
    third = pipe.predict_batch(pages, pages_dev=pages_dev, _maps_override=mo)
    assert seen[2] == (False, True), seen
    assert [key(p) for p in third] == [key(p) for p in second]
    assert any(isinstance(w, CharWord) for p in third for w in p.blocks[0].words)
    pipe.char_details = False
    pipe.predict_batch(pages, pages_dev=pages_dev, _maps_override=mo)
    assert seen[3] == (True, False), seen
