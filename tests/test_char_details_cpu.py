"""Host side of the per-symbol output (no GPU): the frame -> pixel mapping of the attention position, the Char / CharWord result
objects, and the C ABI's declarations of the entry points behind it."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {"msocr_attn_decode", "msocr_attn_beam_alpha_bytes", "msocr_attn_beam_finalize", "msocr_seq_char_details"}


def test_frame_to_pixel_mapping():
    """x = x1 + clamp(8 * centre, 0, new_w) * (x2 - x1) / new_w: the window's ends at centre 0 and T, the clamp where 8 * centre
    runs past the resized width, and a padded canvas (new_w < img_w) that never maps past x2."""
    from manuscript_ocr_amd.recognizers._trba.transforms import FRAME_STRIDE, frame_to_pixel, resized_size
    assert FRAME_STRIDE == 8
    T, img_w = 13, 100
    # a crop that fills the canvas: new_w == img_w; 13 frames x 8 columns = 104 > 100, so centre T clamps onto the right end
    x1, x2, new_w = 40, 240, 100
    assert frame_to_pixel(0.0, new_w, x1, x2) == x1
    assert frame_to_pixel(float(T), new_w, x1, x2) == x2
    assert frame_to_pixel(12.5, new_w, x1, x2) == x2            # 8 * 12.5 = 100 = new_w exactly
    assert frame_to_pixel(12.6, new_w, x1, x2) == x2            # 100.8 > new_w: clamped
    assert frame_to_pixel(6.25, new_w, x1, x2) == 140.0         # column 50 of 100 -> the middle of the window
    assert frame_to_pixel(-0.5, new_w, x1, x2) == x1            # never left of the window either
    # a padded canvas: the resized crop takes 37 of the 100 columns; frames over the padding map onto x2, never past it
    new_w = 37
    xs = frame_to_pixel(np.arange(0, 2 * T + 1) * 0.5, new_w, x1, x2)
    assert xs[0] == x1 and xs.max() == x2 and (np.diff(xs) >= 0).all()
    assert (xs[np.arange(0, 2 * T + 1) * 0.5 * 8 >= new_w] == x2).all()
    assert frame_to_pixel(2.0, new_w, x1, x2) == pytest.approx(x1 + 16 * 200 / 37, abs=1e-9)
    # vectorised over rows as TRBA.chars calls it: [N, steps] centres, [N, 1] windows
    c = np.array([[0.0, 6.25], [13.0, 1.0]])
    got = frame_to_pixel(c, np.array([[100.0], [50.0]]), np.array([[0.0], [10.0]]), np.array([[300.0], [110.0]]))
    assert got.tolist() == [[0.0, 150.0], [110.0, 26.0]]
    # the resized width is ResizeAndPadA's (banker's rounding, at least 1)
    assert resized_size(20, 300, 32, 100) == (100, 7)
    assert resized_size(64, 64, 32, 100) == (32, 32)
    assert resized_size(500, 1, 32, 100) == (1, 32)
    from manuscript_ocr_amd.recognizers._trba.transforms import resize_and_pad
    canvas = resize_and_pad(np.zeros((64, 64, 3), dtype=np.uint8), 32, 100)
    assert (canvas[:, :32] == 0).all() and (canvas[:, 32:] == 255).all()  # pasted at x = 0, new_w columns wide


def test_char_and_charword_validate():
    from pydantic import ValidationError

    from manuscript_ocr_amd.detectors._types import Block, Char, CharWord, Page, Word
    c = Char(char="a", confidence=0.25, x=17.5)
    assert (c.char, c.confidence, c.x) == ("a", 0.25, 17.5)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValidationError):
            Char(char="a", confidence=bad, x=0.0)
    with pytest.raises(ValidationError):
        Char(char="a", confidence=0.5)  # x is required
    poly = [(0.0, 0.0), (10.0, 0.0), (10.0, 5.0), (0.0, 5.0)]
    w = CharWord(polygon=poly, detection_confidence=0.9, text="ab", recognition_confidence=0.5,
                 chars=[c, {"char": "b", "confidence": 1.0, "x": 3.0}])
    assert isinstance(w, Word) and [ch.char for ch in w.chars] == ["a", "b"] and isinstance(w.chars[1], Char)
    assert CharWord(polygon=poly, detection_confidence=0.9).chars == []
    with pytest.raises(ValidationError):
        CharWord(polygon=poly, detection_confidence=0.9, chars=[{"char": "a", "confidence": 2.0, "x": 0.0}])
    with pytest.raises(ValidationError):
        CharWord(polygon=poly, detection_confidence=0.9, recognition_confidence=1.5)
    # Word, Block and Page are what they were: a default dump of a Page holding a CharWord is the dump of the plain Word
    plain = Word(polygon=poly, detection_confidence=0.9, text="ab", recognition_confidence=0.5)
    assert set(Word.model_fields) == {"polygon", "detection_confidence", "text", "recognition_confidence"}
    assert Page(blocks=[Block(words=[w])]).model_dump() == Page(blocks=[Block(words=[plain])]).model_dump()
    assert "chars" in w.model_dump()


def test_header_exports_and_native_list_the_new_symbols():
    import __graft_entry__ as g
    g.build()
    from manuscript_ocr_amd import _native
    header = open(os.path.join(ROOT, "include", "msocr.h")).read()
    declared = set(re.findall(r"\b(msocr_[a-z0-9_]+)\s*\(", header))
    assert NEW_SYMBOLS <= declared, NEW_SYMBOLS - declared
    assert NEW_SYMBOLS <= set(_native.exported_symbols()), NEW_SYMBOLS - set(_native.exported_symbols())
    L = _native.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    # the size helper is plain host arithmetic: [B][steps][beam][T] f32, 0 for a non-positive extent
    assert L.msocr_attn_beam_alpha_bytes(5, 25, 8, 48) == 5 * 25 * 8 * 48 * 4
    assert L.msocr_attn_beam_alpha_bytes(0, 25, 8, 48) == 0 and L.msocr_attn_beam_alpha_bytes(5, 25, 8, 0) == 0
    assert L.msocr_attn_beam_alpha_bytes(2048, 64, 16, 64) == 2048 * 64 * 16 * 64 * 4  # past 2^31
