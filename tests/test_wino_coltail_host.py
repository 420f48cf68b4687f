"""Square tiles + tail column (csrc/winograd.hip, form MSOCR_WINO_4X4_COLTAIL of the shared entry points): the host side, without a GPU.

The tail column of a map with W % 4 == 1 is F(4,3) along H and the three taps along W summed directly, so its weights are
U[xi*3 + kw][co][c] = sum_kh G6[xi][kh] w[co][kh][kw][c] with G6 the Cook-Toom matrix of F(4,3) on {0, +-3/2, +-2/3, inf}.
"""
import ctypes

import numpy as np


def _g6():
    pts = [0.0, 1.5, -1.5, 2 / 3, -2 / 3]
    G6 = np.zeros((6, 3), np.float64)
    for j, a in enumerate(pts):   # G[j] = [1, a, a^2] / prod_{l != j}(a_j - a_l); the point at infinity: [0, 0, 1]
        G6[j] = np.array([1.0, a, a * a]) / np.prod([a - b for l, b in enumerate(pts) if l != j])
    G6[5, 2] = 1.0
    return G6


def _desc(nat, N, H, W, Cin, Cout, stride=1):
    d = nat.ConvDesc()
    d.dtype, d.N, d.H, d.W, d.Cin = nat.F32, N, H, W, Cin
    d.in_sN, d.in_sH, d.in_sW = H * W * Cin, W * Cin, Cin
    d.KH, d.KW, d.stride_h, d.stride_w, d.pad_h, d.pad_w = 3, 3, stride, stride, 1, 1
    d.Ho, d.Wo, d.Cout = (H - 1) // stride + 1, (W - 1) // stride + 1, Cout
    d.out_ld = d.res_ld = Cout
    return d


def test_coltail_weights_host_match_cook_toom_definition():
    """f64, rounded once: within 1 ulp of the einsum (another summation order), the 1.2e-7 * max rule of the other forms.  The form's
    54 planes (ops._wino_weights) are the 4X4 form's 36, then the tail tile's 18; the C call with the form gives the tail tile's and
    writes no more than those."""
    import torch
    from manuscript_ocr_amd import _native as nat
    from manuscript_ocr_amd import ops
    L = nat.lib()
    CT = nat.WINO_4X4_COLTAIL
    rng = np.random.default_rng(41)
    for Cout, Cin in ((32, 16), (64, 96)):
        w = rng.standard_normal((Cout, 3, 3, Cin)).astype(np.float32)  # [Cout][KH][KW][Cin]
        u54 = ops._wino_weights(torch.from_numpy(w), CT).numpy()
        assert u54.shape == (54, Cout, Cin)
        u44 = np.empty((36, Cout, Cin), np.float32)
        assert L.msocr_winograd_weights_host(nat.WINO_4X4, w.ctypes.data, Cout, Cin, u44.ctypes.data) == 0
        assert np.array_equal(u54[:36], u44)
        u = u54[36:54]
        buf = np.full((18 + 1, Cout, Cin), 7.0, np.float32)   # the tail tile's call alone, one sentinel plane behind
        assert L.msocr_winograd_weights_host(CT, w.ctypes.data, Cout, Cin, buf.ctypes.data) == 0
        assert np.array_equal(buf[:18], u) and np.all(buf[18] == 7.0)
        exp = np.einsum("xk,oklc->xloc", _g6(), w.astype(np.float64)).reshape(18, Cout, Cin)
        assert np.abs(u.astype(np.float64) - exp).max() <= 1.2e-7 * np.abs(exp).max()
        # the rows of the points 0 and inf are the kernel's own first and last rows, exactly
        assert np.array_equal(u[0:3], w[:, 0].transpose(1, 0, 2)) and np.array_equal(u[15:18], w[:, 2].transpose(1, 0, 2))
        assert L.msocr_winograd_weights_host(CT, None, Cout, Cin, u.ctypes.data) == -1
        assert L.msocr_winograd_weights_host(CT, w.ctypes.data, Cout, Cin, None) == -1
        assert L.msocr_winograd_weights_host(CT, None, Cout, Cin, None) == -1
        assert L.msocr_winograd_weights_host(CT, w.ctypes.data, 0, Cin, u.ctypes.data) == -1
        assert L.msocr_winograd_weights_host(CT, w.ctypes.data, Cout, 0, u.ctypes.data) == -1


def test_coltail_workspace_bytes_and_shapes_without_the_form():
    """V44 | Mw44 | V41 | Mw41 = (36 * N TH (W // 4) + 18 * N TH) * (Cin + Cout) f32, linear in N; -1 where there is no such form; the
    entry points refuse those shapes before anything is launched."""
    from manuscript_ocr_amd import _native as nat
    L = nat.lib()
    CT = nat.WINO_4X4_COLTAIL
    for N, H, W, Cin, Cout in ((3, 4, 13, 512, 512), (2, 8, 25, 256, 256), (2, 9, 5, 128, 128), (129, 4, 5, 128, 64), (1, 17, 9, 128, 192),
                               (960, 4, 13, 512, 512)):
        TH = -(-H // 4)
        exp = (36 * N * TH * (W // 4) + 18 * N * TH) * (Cin + Cout) * 4
        got = L.msocr_winograd_workspace_bytes(ctypes.byref(_desc(nat, N, H, W, Cin, Cout)), CT)
        assert got == exp, (N, H, W, Cin, Cout)
        assert got == N * L.msocr_winograd_workspace_bytes(ctypes.byref(_desc(nat, 1, H, W, Cin, Cout)), CT)
        assert got < L.msocr_winograd_workspace_bytes(ctypes.byref(_desc(nat, N, H, W, Cin, Cout)), nat.WINO_4X4)
    assert L.msocr_winograd_workspace_bytes(None, CT) == -1
    bad = [_desc(nat, 2, 8, 12, 128, 128), _desc(nat, 2, 8, 14, 128, 128), _desc(nat, 2, 8, 15, 128, 128),   # W % 4 != 1
           _desc(nat, 2, 8, 1, 128, 128),                                                                   # no square tile
           _desc(nat, 2, 8, 13, 144, 128), _desc(nat, 2, 8, 13, 128, 96),                                   # the split GEMMs: Cin % 32, Cout % 64
           _desc(nat, 2, 8, 13, 128, 128, stride=2)]
    bf16 = _desc(nat, 2, 8, 13, 128, 128)
    bf16.dtype = nat.BF16
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below fails its argument checks first
    for d in bad + [bf16]:
        r = ctypes.byref(d)
        assert L.msocr_winograd_workspace_bytes(r, CT) == -1
        assert L.msocr_winograd_input_transform(r, CT, fake, fake, None) == -1
        assert L.msocr_winograd_gemm(r, CT, 1, fake, fake, None) == -1
        assert L.msocr_winograd_output_transform(r, CT, fake, None, None, fake, None) == -1
        assert L.msocr_conv3x3_winograd(r, CT, 1, fake, fake, None, None, fake, fake, None) == -1
    ok = ctypes.byref(_desc(nat, 2, 8, 13, 128, 128))
    assert L.msocr_winograd_input_transform(ok, CT, None, fake, None) == -1
    assert L.msocr_winograd_input_transform(ok, CT, fake, None, None) == -1
    assert L.msocr_winograd_gemm(ok, CT, 1, None, fake, None) == -1      # a null u: one buffer now, the tail column's planes inside it
    assert L.msocr_winograd_gemm(ok, CT, 1, fake, None, None) == -1
    assert L.msocr_winograd_output_transform(ok, CT, None, None, None, fake, None) == -1
    assert L.msocr_winograd_output_transform(ok, CT, fake, None, None, None, None) == -1
    assert L.msocr_conv3x3_winograd(ok, CT, 1, fake, None, None, None, fake, fake, None) == -1
    # split operands only: the form has no exact-f32 GEMM
    assert L.msocr_winograd_gemm(ok, CT, 0, fake, fake, None) == -1
    assert L.msocr_conv3x3_winograd(ok, CT, 0, fake, fake, None, None, fake, fake, None) == -1


def test_crop_lds_bytes_envelope():
    """msocr_winograd_crop_lds_bytes, the rule that decides which SE blocks take the per-crop kernels and how much dynamic LDS they ask
    for: exactly 4 * (H W C + (se ? 4096 + 2C + C/16 : 0)) where the crop (and the SE tail's scratch behind it) fits the 163 840 B of a
    CU, -1 one pixel past each largest fit and wherever the kernels do not apply."""
    from manuscript_ocr_amd import _native as nat
    L = nat.lib()
    SQ, CT = nat.WINO_4X4, nat.WINO_4X4_COLTAIL
    LDS = 160 * 1024

    def lds(d, form, se):
        return L.msocr_winograd_crop_lds_bytes(ctypes.byref(d), form, se)

    def forms(W):  # the square form takes any width (padded last tile), the composite W % 4 == 1 from 5 on
        return (SQ, CT) if W % 4 == 1 and W >= 5 else (SQ,)

    scratch = lambda C: 4096 + 2 * C + C // 16
    # largest H * W that fits with the SE scratch: floor((40960 - scratch) / C)
    assert [(40960 - scratch(C)) // C for C in (64, 128, 256, 512, 1024)] == [573, 285, 141, 69, 33]
    fits = [(3, 7, 64), (5, 6, 128), (6, 9, 128), (7, 3, 64), (4, 1, 64), (1, 33, 1024), (3, 11, 1024), (3, 23, 512), (3, 47, 256),
            (15, 19, 128), (3, 191, 64), (4, 5, 64), (4, 13, 128), (5, 6, 64), (5, 7, 256),   # the shapes of test_gpu_se_block_f64.py
            (4, 13, 512),                                                                      # the workload's
            (8, 17, 256)]                                                                      # test_gpu_se_block_fused.py's largest
    for H, W, C in fits:
        for N in (1, 3):
            d = _desc(nat, N, H, W, C, C)
            for form in forms(W):
                assert lds(d, form, 1) == 4 * (H * W * C + scratch(C)) <= LDS, (H, W, C, form)
                assert lds(d, form, 0) == 4 * H * W * C, (H, W, C, form)
    assert lds(_desc(nat, 2, 8, 17, 256, 256), CT, 1) == 157760
    assert lds(_desc(nat, 2, 1, 33, 1024, 1024), CT, 1) == 160000 and lds(_desc(nat, 2, 3, 23, 512, 512), SQ, 1) == 161920
    # Cin != Cout: the SE kernel only looks at Cout, the chain needs the same plan on both sides
    for form in forms(7):
        assert lds(_desc(nat, 2, 5, 7, 128, 256), form, 1) == 4 * (35 * 256 + scratch(256))
        assert lds(_desc(nat, 2, 5, 7, 128, 256), form, 0) == -1
    assert lds(_desc(nat, 2, 4, 13, 256, 512), CT, 0) == -1 and lds(_desc(nat, 2, 4, 13, 512, 256), SQ, 0) == -1
    # one pixel past each largest fit: no SE kernel; the crop alone still fits, so the chain rule still says yes
    for H, W, C in ((14, 41, 64), (13, 22, 128), (2, 71, 256), (5, 14, 512), (2, 17, 1024)):
        assert H * W == (40960 - scratch(C)) // C + 1
        d = _desc(nat, 2, H, W, C, C)
        for form in forms(W):
            assert 4 * (H * W * C + scratch(C)) > LDS and lds(d, form, 1) == -1, (H, W, C, form)
            assert lds(d, form, 0) == 4 * H * W * C, (H, W, C, form)
    # exactly the LDS of a CU: "fits", not "less than"
    d = _desc(nat, 2, 4, 20, 512, 512)
    assert lds(d, SQ, 0) == LDS == 4 * 4 * 20 * 512 and lds(d, SQ, 1) == -1
    assert lds(_desc(nat, 2, 4, 21, 512, 512), SQ, 0) == -1 and lds(_desc(nat, 2, 4, 21, 512, 512), CT, 0) == -1
    # forms without square tiles
    ok = _desc(nat, 2, 4, 13, 128, 128)
    for se in (0, 1):
        assert lds(ok, nat.WINO_2X2, se) == -1 and lds(ok, nat.WINO_4X2, se) == -1
        assert lds(ok, -1, se) == -1 and lds(ok, CT + 1, se) == -1
        # the composite only where the map has a tail column
        for W in (12, 14, 15, 1, 4):
            assert lds(_desc(nat, 2, 4, W, 128, 128), CT, se) == -1, (W, se)
            assert lds(_desc(nat, 2, 4, W, 128, 128), SQ, se) == 4 * (4 * W * 128 + se * scratch(128)), (W, se)
        assert L.msocr_winograd_crop_lds_bytes(None, SQ, se) == -1 and L.msocr_winograd_crop_lds_bytes(None, CT, se) == -1
        strided = _desc(nat, 2, 8, 13, 128, 128, stride=2)
        assert lds(strided, SQ, se) == -1 and lds(strided, CT, se) == -1
    # the SE tail takes powers of two from 64 to 1024 channels and a dense output
    for C in (32, 96, 192, 2048):
        assert lds(_desc(nat, 1, 1, 1, C, C), SQ, 1) == -1, C
        assert lds(_desc(nat, 1, 1, 1, C, C), SQ, 0) == 4 * C, C      # the chain has no such rule
    for C in (64, 128, 256, 512, 1024):
        assert lds(_desc(nat, 1, 1, 1, C, C), SQ, 1) == 4 * (C + scratch(C)), C
    wide = _desc(nat, 2, 4, 13, 128, 128)
    wide.out_ld = 160
    assert lds(wide, SQ, 1) == -1 and lds(wide, CT, 1) == -1


def test_square_pays_prices_the_tail_column(monkeypatch):
    """ops._square_pays: 36 * (W // 4) + 18 point rows per tile row where the composite runs, 36 * ceil(W / 4) elsewhere or with
    the switch off, against the tall form's 24 * ceil(W / 2)."""
    from manuscript_ocr_amd import ops
    monkeypatch.setattr(ops, "WINOGRAD_COLTAIL", 1)
    assert ops._square_pays(13) and ops._square_pays(25) and ops._square_pays(9)
    assert ops._square_pays(5)            # 54 < 72
    assert not ops._square_pays(1)        # no composite below W = 5: 36 > 24
    assert not ops._square_pays(6) and ops._square_pays(12)   # unchanged: 72 = 72, 108 < 144
    monkeypatch.setattr(ops, "WINOGRAD_COLTAIL", 0)
    assert ops._square_pays(13) and not ops._square_pays(5)   # 144 < 168, 72 = 72
