"""The convolution / GEMM kernels against float64 over their envelope: conv_igemm_kernel (exact f32 and bf16 operands,
csrc/conv_igemm.hip), the split-operand kernels conv_split_pp_kernel (csrc/conv_split_pp.hip) and conv_split_kernel
(csrc/conv_split.hip), and the GEMM stage of every Winograd form (csrc/winograd.hip), reached through ops.conv2d /
ops.attach_split / ops.attach_winograd and, for the batched Winograd GEMMs alone, through the C ABI.  No environment switch is set:
each kernel instance is reached through its shape, and every case of the tables names the instance it must reach (`_instance`
mirrors the host dispatch; a rocprofv3 kernel trace of this module lists the same set).

Reference: `ref` = the convolution in float64 on the CPU (bias, residual and ReLU included), on every output row of small cases and
on sampled rows of large ones (every row of the first, the last and each partial M-tile, the rows on either side of every tile
boundary in one workgroup's list, and 2000 seeded random rows).  A = conv(|x|, |w|) + |b| + |res| in f64, u = 2^-24, K = KH*KW*Cin,
gamma_K = K u / (1 - K u).  The classical bound of the whole f32 sum is gamma_{K+2} * A (the K-term dot product, then the epilogue's
rounded additions of bias and residual); the tests assert the slightly tighter gamma_K * A per element (3 % tighter at K = 64, the
smallest K with an epilogue add here): a stronger condition than rounding theory guarantees, which the measured worst ratio of 0.27
clears with a wide margin.

(a) Exact f32 (conv_igemm_kernel<float>): |dev - ref| <= gamma_K * A per element, and max|dev - ref| <= 4 max|cpu_f32 - ref|
    + 1e-7 scale, cpu_f32 being the same rows in torch-CPU f32 (the convention of test_gpu_f64.py / test_gpu_seq_f64.py).
(b) Split operand (conv_split_pp_kernel, conv_split_kernel; lean and general loaders): max|dev - ref| <= 2 max|exact - ref|
    + 1e-6 scale, `exact` being conv_igemm_kernel<float> on the same case; per element |dev - ref| <= SPLIT_GAMMA * gamma_K * A; and
    rms(dev - ref) <= SPLIT_RMS_FACTOR * rms(exact - ref).  The cases include K = 64 .. 288, where a dropped 2^-18 cross product
    (~2^-19 of a product on average) is 20-30x the f32 rounding: the max bound's 1e-6 slack alone can miss it, the rms bound cannot.
(c) bf16 operands (conv_igemm_kernel<__bf16>): ref on the bf16-rounded x, w and residual; bf16 products are exact in f32 and the
    output is rounded to nearest even once: |dev - ref| <= 2^-8 |ref| (1 + BF16_EPS) + 2 gamma_K A.  2^-8 is the unit roundoff of
    bf16 (8 significant bits: 1 + 2^-8 lies halfway between 1 and the next bf16, 1 + 2^-7), so a correctly rounding store can reach
    it; a truncating store reaches 2^-7 |ref|.
(d) Winograd forms: the rules of test_gpu_ops.py, a bounded multiple of the direct exact kernel's own error (2x2: 4x, tall and the
    fused Cin = 64 kernels: 8x; split GEMMs: 2x their exact twin, square split: 3x the tall split), + (a)'s CPU-f32 bound for the
    exact forms.
(e) Persistent schedule of conv_split_pp_kernel: per pp instance, shapes in each regime of its grid min(roundup8(nblk), n_cu & ~7)
    (nblk <= 7, nblk == grid, nblk == n_cu + 1, >= 3 tiles per workgroup with tilesN >= 2, ktiles 2 and odd, M % BM in {1, BM - 1}),
    each case asserting its own nblk / grid; the batched Winograd GEMMs (nbatch 24 / 36) through msocr_winograd_gemm.
(f) Bitwise invariances (torch.equal): row ranges of a lean launch, images of a general / Winograd launch, the Winograd workspace
    batch split, staged (PROFILE on) against one-call launches, bias=None against zeros, relu against a clamp, and the 2 GB image
    range cut of msocr_conv2d_split.
(g) Guards: every envelope case writes into a channel slice of a wider buffer with channels before and after it and one extra
    image behind the last one, filled with a sentinel that must survive; some read the input / residual from channel slices.

Every case prints its figures under -s: err = max|dev - ref| / scale, the ratio to the exact (or CPU f32) error, the rms ratio and the
worst per-element ratio to its gamma bound."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SEED = 20261016
U32 = 2.0 ** -24
SENTINEL = 7.25
# Bounds, with what the first MI355X run of this module measured (every case prints its figures with -s):
#   exact f32: max err / CPU-f32 err 0.88 .. 1.72; worst per-element err / (gamma_K A) 0.011 .. 0.27.
#   split: max err / exact-kernel err 0.16 .. 1.02 (pp 0.16 .. 0.48, conv_split_kernel 0.50 .. 1.02); rms ratio 0.26 .. 0.84; worst
#     per-element err / (gamma_K A) 0.001 .. 0.078.
#   bf16: worst err / (2^-8 |ref| + 2 gamma_K A) 0.76 .. 0.98 (round to nearest reaches its bound; truncation would read up to 2).
#   Winograd: err / base err 0.34 .. 2.22 (square split against tall split 1.78 .. 2.22, bound 3); exact forms / CPU-f32 err 0.43 .. 1.53.
F32_CPU_FACTOR, F32_CPU_SLACK = 4.0, 1e-7        # exact f32: max err <= 4 CPU-f32 err + 1e-7 scale
SPLIT_EXACT_FACTOR, SPLIT_SLACK = 2.0, 1e-6      # split: max err <= 2 exact-kernel err + 1e-6 scale
SPLIT_RMS_FACTOR = 2.0                           # split: rms err <= 2 exact-kernel rms err
SPLIT_GAMMA = 1.0                                # split: per element <= gamma_K A, as exact f32
BF16_U, BF16_EPS = 2.0 ** -8, 1e-3               # bf16: per element <= 2^-8 |ref| (1 + eps) + 2 gamma_K A
# rule (d), by the form names of WINO_CASES: a form's error against the direct exact kernel's, the square split form's against the
# tall split form's, and the per-layer ceiling (tests/f32_replay.py multiplies these along the chain direct -> tall -> split -> square)
WINO_DIRECT_FACTOR, WINO_DIRECT_SLACK = {"2x2": 4, "42": 8, "f64": 8, "f64s": 8}, 1e-6
SQUARE_TALL_FACTOR, SQUARE_TALL_SLACK = 3.0, 1e-7
WINO_CEILING = 2e-5                              # every form: max err <= 2e-5 scale
LARGE_FLOP = 1e9                                 # above this the f64 reference runs on sampled rows
N_RANDOM_ROWS = 2000


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from manuscript_ocr_amd import ops as _ops
    return _ops


def _gamma(K):
    return K * U32 / (1 - K * U32)


def _n_cu():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    return n & ~7 if n > 8 else 8


# ------------------------------------------------------------------------------------------------ instance selection (host mirror)
def _instance(mode, Cin, Cout, k, stride, pad, res, lean_layout=True):
    """The kernel instance the host dispatch picks (csrc/conv_igemm.hip launch_typed, csrc/conv_split.hip launch_split_one,
    csrc/conv_split_pp.hip msocr_internal_split_pp_launch, ops.conv2d's lean test)."""
    one = tuple(k) == (1, 1) and tuple(pad) == (0, 0)
    if mode == "split":
        lean = "lean" if one and tuple(stride) == (1, 1) and lean_layout else "gen"
        K = k[0] * k[1] * Cin
        if Cout % 128 == 0 and not res and K >= 64:
            return f"pp<{'2,4' if Cout % 256 == 0 else '4,2'},{lean}>"
        return f"split<{128 if Cout % 128 == 0 else 64},{lean}>"
    es = 4 if mode == "f32" else 2
    wide = "wide" if (Cin * es) % 128 == 0 else "narrow"
    cls = 128 if Cout % 128 == 0 else (64 if Cout % 64 == 0 else 32)
    lean = ",lean" if mode == "f32" and one and wide == "wide" and cls in (128, 64) else ""
    return f"{mode}<{cls},{wide}{lean}>"


def _pp_geometry(M, Cout, K, inst, nbatch=1):
    """conv_split_pp_kernel's tile list (launch_pp + the kernel's XCD-contiguous static schedule): BM, tiles, nblk, grid and each
    workgroup's tile numbers."""
    TM, TN = (2, 4) if inst.startswith("pp<2,4") else (4, 2)
    BM, BN = 64 * TM, 64 * TN
    tilesM, tilesN = -(-M // BM), Cout // BN
    nblk = tilesM * tilesN * nbatch
    grid = min((nblk + 7) & ~7, _n_cu())
    per_x, xq, xr = grid >> 3, nblk >> 3, nblk & 7
    lists = []
    for b in range(grid):
        xcd, slot = b & 7, b >> 3
        x_start = xcd * (xq + 1) if xcd < xr else xr * (xq + 1) + (xcd - xr) * xq
        x_cnt = xq + (1 if xcd < xr else 0)
        my = (x_cnt - slot + per_x - 1) // per_x if slot < x_cnt else 0
        lists.append([x_start + slot + n * per_x for n in range(my)])
    return dict(BM=BM, BN=BN, tilesM=tilesM, tilesN=tilesN, nblk=nblk, grid=grid, ktiles=K // 32, lists=lists)


def _check_regime(geo, regime, M):
    BM, nblk, grid, kt = geo["BM"], geo["nblk"], geo["grid"], geo["ktiles"]
    mine = [len(t) for t in geo["lists"]]
    for r in regime.split("+"):
        if r == "few":
            assert nblk <= 7, (r, nblk)
        elif r == "eqgrid":
            assert nblk == grid, (r, nblk, grid)
        elif r == "cu1":
            assert nblk == _n_cu() + 1 and nblk % 8 != 0, (r, nblk)
        elif r == "multi":
            assert min(mine) >= 3 and max(mine) >= 5 and geo["tilesN"] >= 2, (r, min(mine), max(mine), geo["tilesN"])
            # the tiles of one workgroup must differ in tile_n, or every bias slot holds the same values and a wrong slot reads right
            nb1 = geo["tilesM"] * geo["tilesN"]
            spans = sum(len({(t % nb1) % geo["tilesN"] for t in ts}) > 1 for ts in geo["lists"])
            assert spans == len(geo["lists"]), (r, "workgroups whose tiles span several tile_n", spans, len(geo["lists"]))
        elif r == "kt2":
            assert kt == 2, (r, kt)
        elif r == "ktodd":
            assert kt % 2 == 1 and {(m * kt) % 2 for m in mine if m} == {0, 1}, (r, kt, set(mine))
        elif r == "m1":
            assert M % BM == 1, (r, M, BM)
        elif r == "mlast":
            assert M % BM == BM - 1, (r, M, BM)
        else:
            raise ValueError(r)


def _sample_rows(M, geo, BM, g):
    """Every row of the first, the last and each partial M-tile, both sides of every tile boundary in workgroup 0's list, random rows."""
    rows = [torch.arange(0, min(BM, M)), torch.arange(max(0, (M - 1) // BM * BM - BM), M)]
    if geo is not None:
        tn = geo["tilesN"] * geo["tilesM"]
        for t in geo["lists"][0]:
            tm = (t % tn) // geo["tilesN"]
            for r in (tm * BM - 1, tm * BM, tm * BM + BM - 1, tm * BM + BM):
                if 0 <= r < M:
                    rows.append(torch.tensor([r]))
    rows.append(torch.randint(0, M, (N_RANDOM_ROWS,), generator=g))
    return torch.unique(torch.cat(rows))


# ------------------------------------------------------------------------------------------------ f64 reference on output rows
def _gather_patches(x, rows, Ho, Wo, k, stride, pad):
    """x [N,H,W,C] (any device, any dtype) -> f64 CPU patches [R, KH*KW*C] of flat output rows `rows` (zeros outside the image)."""
    N, H, W, C = x.shape
    KH, KW = k
    rows_d = rows.to(x.device)
    n = rows_d // (Ho * Wo)
    rem = rows_d % (Ho * Wo)
    ho, wo = rem // Wo, rem % Wo
    hi = ho[:, None] * stride[0] - pad[0] + torch.arange(KH, device=x.device)[None]
    wi = wo[:, None] * stride[1] - pad[1] + torch.arange(KW, device=x.device)[None]
    ok = ((hi >= 0) & (hi < H))[:, :, None] & ((wi >= 0) & (wi < W))[:, None, :]
    p = x[n[:, None, None], hi.clamp(0, H - 1)[:, :, None], wi.clamp(0, W - 1)[:, None, :]]   # [R, KH, KW, C]
    p = p.float().cpu().double() * ok.cpu()[..., None]
    return p.reshape(len(rows), KH * KW * C)


def _rows_of(t, rows, Ho, Wo):
    """Output rows of an NHWC tensor / view -> f64 CPU [R, C]."""
    rows_d = rows.to(t.device)
    n, rem = rows_d // (Ho * Wo), rows_d % (Ho * Wo)
    return t[n, rem // Wo, rem % Wo].float().cpu().double()


def _reference(x, w, b, res, relu, rows, Ho, Wo, stride, pad):
    """ref, A (f64) and the torch-CPU f32 result on the given output rows."""
    Cout, KH, KW, Cin = w.shape
    P = _gather_patches(x, rows, Ho, Wo, (KH, KW), stride, pad)
    wm = w.float().cpu().double().reshape(Cout, -1)
    ref = P @ wm.t()
    A = P.abs() @ wm.abs().t()
    cpu = (P.float() @ wm.float().t())
    if b is not None:
        ref = ref + b.cpu().double()
        A = A + b.cpu().double().abs()
        cpu = cpu + b.cpu().float()
    if res is not None:
        r = _rows_of(res, rows, Ho, Wo)
        ref, A, cpu = ref + r, A + r.abs(), cpu + r.float()
    if relu:
        ref, cpu = ref.clamp_min(0), cpu.clamp_min(0)
    return ref, A, cpu.double()


def _guarded_out(N, Ho, Wo, Cout, dtype, pre, post):
    """An output view with `pre` / `post` sentinel channels around it and one sentinel image behind the last one."""
    buf = torch.full((N + 1, Ho, Wo, pre + Cout + post), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[:N, :, :, pre:pre + Cout]


def _check_guard(buf, N, pre, Cout, what):
    assert torch.all(buf[:, :, :, :pre] == SENTINEL), (what, "channels before the output were written")
    assert torch.all(buf[:, :, :, pre + Cout:] == SENTINEL), (what, "channels after the output were written")
    assert torch.all(buf[N:] == SENTINEL), (what, "rows past M were written")


# ------------------------------------------------------------------------------------------------ (a)-(c), (e), (g): direct cases
def _gen_shape(tilesM, BM, r, exact_r=True):
    """(1, H, W) with H * W = (tilesM - 1) * BM + r and an odd W < 256 (a 3x3 / 1 / 1 map of exactly that many pixels); exact_r=False
    moves r to the next odd value with such a W."""
    for rr in ([r] if exact_r else range(r, BM, 2)):
        M = (tilesM - 1) * BM + rr
        for W in range(3, 256, 2):
            if M % W == 0:
                return (1, M // W, W)
    raise AssertionError((tilesM, BM, r))


def _pp_cases():
    """Per pp instance, shapes in each schedule regime.  lean: 1x1 over N = 1, H = M, W = 1; gen: 3x3 / 1 / 1 (K = 288, 9 K-tiles)
    or a 1x1 over a pixel-strided view (K = 64, 2 K-tiles).  Built from the CU count at collection time (pytest collects on the GPU box)."""
    ncu = _n_cu() if torch.cuda.is_available() else 256
    out = []
    # tn = tilesN = 3 for both instances: with grid 256 a workgroup's tiles are 32 apart, so an even tilesN would give all of them the
    # same tile_n (one set of bias values in every slot); 3 makes consecutive tiles of a workgroup cycle through the tile_n
    for tmtn, cout1, tn in (("2,4", 256, 3), ("4,2", 128, 3)):
        BM = 128 if tmtn == "2,4" else 256
        many = -(-(9 * ncu // 2) // tn)         # tilesM for ~4.5 tiles per workgroup
        for regime, tilesM, tilesN, r, Cin in (("few+kt2+m1", 5, 1, 1, 64), ("eqgrid+mlast", 8, tn, BM - 1, 96),
                                               ("cu1+ktodd+m1", ncu + 1, 1, 1, 96), ("multi+kt2+mlast", many, tn, BM - 1, 64)):
            M = (tilesM - 1) * BM + r
            out.append(dict(name=f"pp{tmtn}-lean-{regime}", inst=f"pp<{tmtn},lean>", mode="split", shape=(1, M, 1), Cin=Cin,
                            Cout=cout1 * tilesN, k=(1, 1), stride=(1, 1), pad=(0, 0), relu=True, res=None, regime=regime))
        for regime, tilesM, tilesN, r, k in (("few+kt2+m1", 5, 1, 1, (1, 1)), ("eqgrid+mlast", 8, tn, BM - 1, (3, 3)),
                                             ("cu1+ktodd", ncu + 1, 1, 1, (3, 3)), ("multi", many, tn, 1, (3, 3))):
            if k == (1, 1):
                shape, Cin, pad = (1, (tilesM - 1) * BM + r, 1), 64, (0, 0)
            else:
                shape, Cin, pad = _gen_shape(tilesM, BM, r, exact_r=regime.endswith(("m1", "mlast"))), 32, (1, 1)
            out.append(dict(name=f"pp{tmtn}-gen-{regime}", inst=f"pp<{tmtn},gen>", mode="split", shape=shape, Cin=Cin,
                            Cout=cout1 * tilesN, k=k, stride=(1, 1), pad=pad, relu=False, res=None, regime=regime,
                            wcols=2 if k == (1, 1) else 1))
    return out


def _c(name, inst, mode, shape, Cin, Cout, k, stride, pad, relu=False, res=None, in_extra=0, bias=True):
    return dict(name=name, inst=inst, mode=mode, shape=shape, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=pad, relu=relu, res=res,
                in_extra=in_extra, bias=bias)


# res: None, "dense" (res_ld == Cout) or "slice" (a channel slice of a buffer 32 channels wider: res_ld > out_ld of the guard)
ENVELOPE = [
    # exact f32: the eight conv_igemm_kernel<float> instances of launch_typed (wide = Cin % 32 == 0, lean = 1x1 without padding)
    _c("f32-128-wide-lean", "f32<128,wide,lean>", "f32", (2, 9, 13), 64, 128, (1, 1), (1, 1), (0, 0), True, "dense"),
    _c("f32-128-wide-lean-s2", "f32<128,wide,lean>", "f32", (2, 10, 15), 64, 256, (1, 1), (2, 2), (0, 0), False, None),
    _c("f32-128-wide", "f32<128,wide>", "f32", (2, 11, 7), 32, 256, (3, 3), (1, 1), (1, 1), True, None, in_extra=32),
    _c("f32-128-narrow", "f32<128,narrow>", "f32", (1, 15, 17), 16, 128, (3, 3), (2, 2), (1, 1), False, "slice"),
    _c("f32-128-narrow-1x1", "f32<128,narrow>", "f32", (3, 5, 7), 48, 128, (1, 1), (1, 1), (0, 0), True, None),
    _c("f32-64-wide-lean", "f32<64,wide,lean>", "f32", (2, 8, 9), 96, 192, (1, 1), (1, 1), (0, 0), True, "slice"),
    _c("f32-64-wide", "f32<64,wide>", "f32", (2, 12, 10), 32, 64, (2, 2), (2, 2), (0, 0), False, None),
    _c("f32-64-narrow", "f32<64,narrow>", "f32", (1, 13, 11), 16, 64, (3, 3), (1, 1), (1, 1), True, "dense"),
    _c("f32-64-narrow-1x1", "f32<64,narrow>", "f32", (2, 6, 7), 16, 64, (1, 1), (1, 1), (0, 0), False, None),
    _c("f32-32-wide", "f32<32,wide>", "f32", (2, 9, 11), 32, 96, (3, 3), (1, 1), (1, 1), True, None, in_extra=32),
    _c("f32-32-wide-1x1", "f32<32,wide>", "f32", (1, 17, 9), 64, 32, (1, 1), (1, 1), (0, 0), False, "dense"),
    _c("f32-32-narrow", "f32<32,narrow>", "f32", (2, 14, 9), 48, 32, (1, 1), (2, 2), (0, 0), True, None),
    # bf16: the six conv_igemm_kernel<__bf16> instances (wide = Cin % 64 == 0)
    _c("bf16-128-wide", "bf16<128,wide>", "bf16", (2, 9, 13), 64, 128, (1, 1), (1, 1), (0, 0), True, "dense"),
    _c("bf16-128-narrow", "bf16<128,narrow>", "bf16", (1, 15, 13), 32, 256, (3, 3), (2, 2), (1, 1), False, None),
    _c("bf16-64-wide", "bf16<64,wide>", "bf16", (2, 7, 9), 128, 64, (3, 3), (1, 1), (1, 1), True, "slice"),
    _c("bf16-64-narrow", "bf16<64,narrow>", "bf16", (2, 8, 11), 96, 192, (1, 1), (1, 1), (0, 0), False, None, in_extra=32),
    _c("bf16-32-wide", "bf16<32,wide>", "bf16", (1, 12, 10), 64, 32, (3, 3), (1, 1), (1, 1), False, None),
    _c("bf16-32-narrow", "bf16<32,narrow>", "bf16", (2, 10, 14), 32, 96, (2, 2), (2, 2), (0, 0), True, "dense"),
    # split operand: every pp instance and conv_split_kernel<BN, 3, GEN> at short K (64 .. 288)
    _c("split-pp24-lean", "pp<2,4,lean>", "split", (2, 9, 13), 64, 256, (1, 1), (1, 1), (0, 0), True, None),
    _c("split-pp24-gen", "pp<2,4,gen>", "split", (1, 15, 17), 32, 512, (3, 3), (2, 2), (1, 1), False, None, in_extra=32),
    _c("split-pp42-lean", "pp<4,2,lean>", "split", (3, 7, 11), 96, 128, (1, 1), (1, 1), (0, 0), False, None, in_extra=32),
    _c("split-pp42-gen", "pp<4,2,gen>", "split", (2, 12, 10), 64, 384, (2, 2), (2, 2), (0, 0), True, None),
    _c("split-128-lean-res", "split<128,lean>", "split", (2, 9, 13), 64, 128, (1, 1), (1, 1), (0, 0), True, "slice"),
    _c("split-128-lean-k32", "split<128,lean>", "split", (2, 11, 9), 32, 256, (1, 1), (1, 1), (0, 0), False, None),
    _c("split-128-gen-res", "split<128,gen>", "split", (1, 13, 11), 32, 128, (3, 3), (1, 1), (1, 1), False, "slice"),
    _c("split-128-gen-k32", "split<128,gen>", "split", (2, 10, 12), 32, 256, (1, 1), (2, 2), (0, 0), True, None),
    _c("split-64-lean", "split<64,lean>", "split", (2, 8, 7), 128, 192, (1, 1), (1, 1), (0, 0), True, None),
    _c("split-64-lean-res", "split<64,lean>", "split", (1, 16, 9), 64, 64, (1, 1), (1, 1), (0, 0), False, "slice", in_extra=32),
    _c("split-64-gen-res", "split<64,gen>", "split", (2, 11, 9), 64, 64, (3, 3), (2, 2), (1, 1), True, "slice"),
    _c("split-64-gen", "split<64,gen>", "split", (1, 12, 13), 32, 192, (3, 3), (1, 1), (1, 1), False, None),
    _c("split-pp24-lean-nobias", "pp<2,4,lean>", "split", (1, 21, 23), 64, 256, (1, 1), (1, 1), (0, 0), False, None, bias=False),
] + _pp_cases()


def _make_inputs(c, g):
    N, H, W = c["shape"]
    Cin, Cout, (KH, KW) = c["Cin"], c["Cout"], c["k"]
    dt = torch.bfloat16 if c["mode"] == "bf16" else torch.float32
    # wcols > 1: the map is the first W columns of a wider one, so its pixels are no dense sequence (the general loader on a 1x1 / 1 / 0)
    xbuf = torch.randn(N, H, W * c.get("wcols", 1), Cin + c.get("in_extra", 0), generator=g, device="cuda")
    x = xbuf.to(dt)[:, :, :W, c.get("in_extra", 0):]
    w = (torch.randn(Cout, KH, KW, Cin, generator=g, device="cuda") * (2.0 / (KH * KW * Cin)) ** 0.5).to(dt).contiguous()
    b = torch.randn(Cout, generator=g, device="cuda") * 0.5 if c.get("bias", True) else None   # a distinct bias per channel
    return x, w, b


def _pad_ho(c):
    N, H, W = c["shape"]
    (KH, KW), (sh, sw), (ph, pw) = c["k"], c["stride"], c["pad"]
    return (H + 2 * ph - KH) // sh + 1, (W + 2 * pw - KW) // sw + 1


def _conv(ops, x, w, b, c, out=None, res=None, relu=None):
    return ops.conv2d(x, w, b, c["stride"], c["pad"], c["relu"] if relu is None else relu, res, out=out)


@pytest.mark.parametrize("c", ENVELOPE, ids=lambda c: c["name"])
def test_conv_envelope(ops, c, monkeypatch):
    monkeypatch.setattr(ops, "SPLIT_MIN_K", 0)
    monkeypatch.setattr(ops, "SPLIT_BF16X3", 1)
    g = torch.Generator(device="cuda").manual_seed(SEED + sum(map(ord, c["name"])))
    gc = torch.Generator().manual_seed(SEED)
    N, H, W = c["shape"]
    Cin, Cout, mode = c["Cin"], c["Cout"], c["mode"]
    Ho, Wo = _pad_ho(c)
    M, K = N * Ho * Wo, c["k"][0] * c["k"][1] * Cin
    x, w, b = _make_inputs(c, g)
    dt = x.dtype
    res = None
    if c["res"] is not None:
        extra = 32 if c["res"] == "slice" else 0
        res = torch.randn(N, Ho, Wo, Cout + extra, generator=g, device="cuda").to(dt)[..., :Cout]
    lean_layout = c.get("wcols", 1) == 1
    inst = _instance(mode, Cin, Cout, c["k"], c["stride"], c["pad"], res is not None, lean_layout)
    assert inst == c["inst"], (inst, c["inst"])
    geo = None
    if inst.startswith("pp"):
        geo = _pp_geometry(M, Cout, K, inst)
        if "regime" in c:
            _check_regime(geo, c["regime"], M)
    pre = post = 8 if dt == torch.bfloat16 else 4
    if res is not None and c["res"] == "slice":
        assert res.stride(2) > Cout + pre + post   # res_ld > out_ld: the residual cases of conv_split_kernel read with res_ld
    w_dev = ops.attach_split(w, False) if mode != "split" else w
    buf, out = _guarded_out(N, Ho, Wo, Cout, dt, pre, post)
    ops.PROFILE = []
    _conv(ops, x, w_dev, b, c, out=out, res=res)
    tags = [t[4][3] for t in ops.PROFILE]
    ops.PROFILE = None
    assert tags == ["direct_split" if mode == "split" else "direct"], tags
    torch.cuda.synchronize()
    _check_guard(buf, N, pre, Cout, c["name"])

    BM = geo["BM"] if geo else 128
    rows = torch.arange(M) if 2.0 * M * Cout * K <= LARGE_FLOP else _sample_rows(M, geo, BM, gc)
    ref, A, cpu = _reference(x, w, b, res, c["relu"], rows, Ho, Wo, c["stride"], c["pad"])
    dev = _rows_of(out, rows, Ho, Wo)
    scale = max(ref.abs().max().item(), 1.0)
    e = (dev - ref).abs()
    err = e.max().item()
    gam = _gamma(K)
    if mode == "f32":
        e_cpu = (cpu - ref).abs().max().item()
        worst = (e / (gam * A).clamp_min(1e-300)).max().item()
        print(f"{c['name']} [{inst}] rows {len(rows)}/{M}: err {err / scale:.2e}, / cpu-f32 err {err / max(e_cpu, 1e-300):.2f}, "
              f"worst / gamma_K A {worst:.3f}")
        assert torch.all(e <= gam * A), (c["name"], worst)
        assert err <= F32_CPU_FACTOR * e_cpu + F32_CPU_SLACK * scale, (err, e_cpu, scale)
    elif mode == "split":
        exact = _conv(ops, x, ops.attach_split(w.clone(), False), b, c, res=res)
        torch.cuda.synchronize()
        ee = (_rows_of(exact, rows, Ho, Wo) - ref)
        e_ex, rms_ex = ee.abs().max().item(), ee.pow(2).mean().sqrt().item()
        rms = (dev - ref).pow(2).mean().sqrt().item()
        worst = (e / (gam * A).clamp_min(1e-300)).max().item()
        print(f"{c['name']} [{inst}] rows {len(rows)}/{M}: err {err / scale:.2e}, / exact err {err / max(e_ex, 1e-300):.2f}, "
              f"rms / exact rms {rms / max(rms_ex, 1e-300):.2f}, worst / gamma_K A {worst:.3f}"
              + (f", nblk {geo['nblk']} grid {geo['grid']} tiles/wg {min(map(len, geo['lists']))}-{max(map(len, geo['lists']))}"
                 f" ktiles {geo['ktiles']}" if geo else ""))
        assert err <= SPLIT_EXACT_FACTOR * e_ex + SPLIT_SLACK * scale, (err, e_ex, scale)
        assert rms <= SPLIT_RMS_FACTOR * rms_ex, (rms, rms_ex)
        assert torch.all(e <= SPLIT_GAMMA * gam * A), (c["name"], worst)
    else:
        lim = BF16_U * ref.abs() * (1 + BF16_EPS) + 2 * gam * A
        worst = (e / lim.clamp_min(1e-300)).max().item()
        print(f"{c['name']} [{inst}] rows {len(rows)}/{M}: err {err / scale:.2e}, worst / (2^-8 |ref| + 2 gamma_K A) {worst:.3f}")
        assert torch.all(e <= lim), (c["name"], worst)


# ------------------------------------------------------------------------------------------------ (d), (g): Winograd forms
# form: "2x2" exact, "42" tall exact, "42s" tall split, "44s" square split, "f64" fused Cin = 64 exact, "f64s" fused split
WINO_CASES = [
    # name, form, N, H, W, Cin, Cout, relu, res, pool
    ("w22-exact", "2x2", 2, 9, 13, 128, 128, True, "slice", False),
    ("w22-exact-c96", "2x2", 1, 7, 11, 128, 96, False, None, False),
    ("w42-exact", "42", 2, 13, 9, 128, 256, False, "slice", False),
    ("w42-split-pp", "42s", 2, 13, 9, 128, 256, True, None, False),
    ("w42-split-pp42", "42s", 1, 17, 11, 160, 128, False, "slice", False),
    ("w42-split-64", "42s", 2, 11, 10, 128, 192, True, None, False),
    ("w44-split-pp", "44s", 2, 13, 15, 128, 256, True, "slice", False),
    ("w44-split-64", "44s", 1, 9, 17, 128, 64, False, None, False),
    ("f64-v1-exact", "f64", 2, 8, 14, 64, 128, True, None, False),
    ("f64-v1-exact-pool", "f64", 2, 8, 14, 64, 96, True, None, True),
    ("f64-v1-split", "f64s", 2, 9, 13, 64, 160, False, "slice", False),
    ("f64-v1-split-pool", "f64s", 1, 12, 10, 64, 160, True, None, True),
    ("f64-v2-split", "f64s", 2, 9, 13, 64, 128, True, "slice", False),
    ("f64-v2-split-pool", "f64s", 1, 12, 10, 64, 128, True, None, True),
]


def _wino_weights(ops, w, form, monkeypatch):
    """Attach the form's transform-domain weights to a copy of w and set the dispatch so that conv2d takes `form`; returns the
    weight and the PROFILE tag it must produce."""
    monkeypatch.setattr(ops, "_tall_pays", lambda H: True)
    monkeypatch.setattr(ops, "WINOGRAD_TALL", 0 if form == "2x2" else 1)
    monkeypatch.setattr(ops, "WINOGRAD_SQUARE", 1 if form == "44s" else 0)
    monkeypatch.setattr(ops, "WINOGRAD_SQUARE_MIN_CIN", 128)
    monkeypatch.setattr(ops, "_square_pays", lambda W: True)
    monkeypatch.setattr(ops, "SPLIT_BF16X3", 1)
    split = form.endswith("s")
    wk = ops.attach_winograd(w.clone(), split)
    if form.startswith("f64"):
        assert (getattr(wk, "_msocr_wino42_fused_split", None) is not None) == split
        return wk, "winograd42_fused" + ("_split" if split else "")
    return wk, {"2x2": "winograd", "42": "winograd42", "42s": "winograd42_split", "44s": "winograd44_split"}[form]


def _wino_inputs(case, g):
    name, form, N, H, W, Cin, Cout, relu, res, pool = case
    x = torch.randn(N, H, W, Cin, generator=g, device="cuda")
    w = torch.randn(Cout, 3, 3, Cin, generator=g, device="cuda") * (2.0 / (Cin * 9)) ** 0.5
    b = torch.randn(Cout, generator=g, device="cuda") * 0.5
    r = torch.randn(N, H, W, Cout + 32, generator=g, device="cuda")[..., :Cout] if res else None
    return x, w, b, r


def _f64_conv3x3(x, w, b, r, relu, pool):
    ref = F.conv2d(x.cpu().double().permute(0, 3, 1, 2), w.cpu().double().permute(0, 3, 1, 2), b.cpu().double(), padding=1)
    cpu = F.conv2d(x.cpu().permute(0, 3, 1, 2), w.cpu().permute(0, 3, 1, 2), b.cpu(), padding=1)
    if r is not None:
        ref, cpu = ref + r.cpu().double().permute(0, 3, 1, 2), cpu + r.cpu().permute(0, 3, 1, 2)
    if relu:
        ref, cpu = F.relu(ref), F.relu(cpu)
    full = ref
    if pool:
        ref, cpu = F.max_pool2d(ref, 2, 2), F.max_pool2d(cpu, 2, 2)
    return ref.permute(0, 2, 3, 1), cpu.permute(0, 2, 3, 1).double(), full


@pytest.mark.parametrize("case", WINO_CASES, ids=lambda c: c[0])
def test_winograd_envelope(ops, case, monkeypatch):
    name, form, N, H, W, Cin, Cout, relu, res, pool = case
    g = torch.Generator(device="cuda").manual_seed(SEED + sum(map(ord, name)))
    x, w, b, r = _wino_inputs(case, g)
    wk, tag = _wino_weights(ops, w, form, monkeypatch)
    oh, ow = (H // 2, W // 2) if pool else (H, W)
    buf, out = _guarded_out(N, oh, ow, Cout, torch.float32, 4, 4)
    ops.PROFILE = []
    ops.conv2d(x, wk, b, (1, 1), (1, 1), relu, r, out=out, pool2=pool)
    tags = [t[4][3] for t in ops.PROFILE if t[2] == "conv_gemm"]
    ops.PROFILE = None
    assert tags == [tag], tags
    torch.cuda.synchronize()
    _check_guard(buf, N, 4, Cout, name)
    ref, cpu, full = _f64_conv3x3(x, w, b, r, relu, pool)
    scale = max(full.abs().max().item(), 1.0)
    err = (out.cpu().double() - ref).abs().max().item()

    def err_of(o):
        o = o.cpu().double()
        if pool:
            o = F.max_pool2d(o.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        return (o - ref).abs().max().item()

    direct = ops.conv2d(x, ops.attach_split(w.clone(), False), b, (1, 1), (1, 1), relu, r)
    e_d = err_of(direct)
    if form in WINO_DIRECT_FACTOR:
        base, factor, slack = e_d, WINO_DIRECT_FACTOR[form], WINO_DIRECT_SLACK
    else:   # split GEMMs: against the exact twin of the same form (tall), the square form against the tall split form
        twin = "42" if form == "42s" else "42s"
        wt, _ = _wino_weights(ops, w, twin, monkeypatch)
        base = err_of(ops.conv2d(x, wt, b, (1, 1), (1, 1), relu, r))
        factor, slack = (SPLIT_EXACT_FACTOR, SPLIT_SLACK) if form == "42s" else (SQUARE_TALL_FACTOR, SQUARE_TALL_SLACK)
    e_cpu = (cpu - ref).abs().max().item()
    print(f"{name} [{tag}]: err {err / scale:.2e}, / base err {err / max(base, 1e-300):.2f} (bound {factor}), "
          f"/ direct err {err / max(e_d, 1e-300):.2f}, / cpu-f32 err {err / max(e_cpu, 1e-300):.2f}")
    assert err <= WINO_CEILING * scale and err <= factor * base + slack * scale, (err, base, scale)
    if form in ("2x2", "42", "f64"):
        assert err <= F32_CPU_FACTOR * e_cpu + F32_CPU_SLACK * scale, (err, e_cpu, scale)


# ------------------------------------------------------------------------------------------------ (e): batched Winograd GEMMs (pp)
WINO_GEMM_CASES = [
    # form, P, Cin, Cout, Mt target residue (1 or BM - 1), tilesM: the partial M tile of every point is not its workgroup's last tile
    ("42", 24, 64, 128, "m1", 16),
    ("42", 24, 96, 128, "mlast", 17),
    ("44", 36, 64, 256, "m1", 8),
    ("44", 36, 96, 256, "mlast", 9),
]


@pytest.mark.parametrize("case", WINO_GEMM_CASES, ids=lambda c: f"{c[0]}-cin{c[2]}-{c[4]}")
def test_winograd_gemm_pp_geometry(ops, case):
    """msocr_winograd_gemm (split) on random V / U: nbatch = P GEMMs of Mt x Cout x Cin in one conv_split_pp_kernel launch, sampled
    rows of every point against f64 and against exact f32 (the 1x1 exact kernel on the same point); the workspace tail behind Mw
    (one extra row of the last point) holds a sentinel."""
    from manuscript_ocr_amd import _native as nat
    form, P, Cin, Cout, reg, tilesM = case
    inst = "pp<2,4,lean>" if Cout % 256 == 0 else "pp<4,2,lean>"
    BM = 128 if Cout % 256 == 0 else 256
    Mt = (tilesM - 1) * BM + (1 if reg == "m1" else BM - 1)
    geo = _pp_geometry(Mt, Cout, Cin, inst, nbatch=P)
    _check_regime(geo, reg, Mt)
    assert geo["nblk"] > geo["grid"] and min(map(len, geo["lists"])) >= 1
    nblk1 = geo["tilesM"] * geo["tilesN"]
    partial_not_last = [ts for ts in geo["lists"] if any((t % nblk1) // geo["tilesN"] == geo["tilesM"] - 1 for t in ts[:-1])]
    assert partial_not_last, "no workgroup holds a partial M tile before another tile"
    fid = nat.WINO_4X2 if form == "42" else nat.WINO_4X4
    mw = 2 if form == "42" else 4
    d = nat.ConvDesc()
    d.dtype, d.N, d.H, d.W, d.Cin = nat.F32, 1, 4, mw * Mt, Cin
    d.in_sN, d.in_sH, d.in_sW = 4 * mw * Mt * Cin, mw * Mt * Cin, Cin
    d.KH, d.KW, d.stride_h, d.stride_w, d.pad_h, d.pad_w = 3, 3, 1, 1, 1, 1
    d.Ho, d.Wo, d.Cout, d.out_ld, d.res_ld, d.flags = 4, mw * Mt, Cout, Cout, 0, 0
    L = nat.lib()
    nbytes = L.msocr_winograd_workspace_bytes(ctypes.byref(d), fid)
    assert nbytes == 4 * P * Mt * (Cin + Cout)
    g = torch.Generator(device="cuda").manual_seed(SEED + Mt)
    tail = 4 * Cout
    ws = torch.full((P * Mt * (Cin + Cout) + tail,), SENTINEL, device="cuda")
    V = ws[:P * Mt * Cin].view(P, Mt, Cin)
    V.copy_(torch.randn(P, Mt, Cin, generator=g, device="cuda"))
    u = torch.randn(P, Cout, Cin, generator=g, device="cuda") * Cin ** -0.5
    planes = ops.split_planes_ktile(u, P, Cout)
    nat.check(L.msocr_winograd_gemm(ctypes.byref(d), fid, 1, planes.data_ptr(), ws.data_ptr(), ops._stream()), "winograd_gemm")
    torch.cuda.synchronize()
    assert torch.all(ws[P * Mt * (Cin + Cout):] == SENTINEL), "written past Mw"
    Mw = ws[P * Mt * Cin:P * Mt * (Cin + Cout)].view(P, Mt, Cout)
    gc = torch.Generator().manual_seed(SEED)
    rows = _sample_rows(Mt, None, BM, gc)
    gam = _gamma(Cin)
    worst_r = worst_g = worst_rms = 0.0
    for p in range(P):
        a = V[p, rows].cpu().double()
        ud = u[p].cpu().double()
        ref, A = a @ ud.t(), a.abs() @ ud.abs().t()
        exact = ops.conv2d(V[p].view(1, Mt, 1, Cin), ops.attach_split(u[p].reshape(Cout, 1, 1, Cin).clone(), False), None)
        ee = exact[0, rows.cuda(), 0].cpu().double() - ref
        e = Mw[p, rows].cpu().double() - ref
        scale = max(ref.abs().max().item(), 1.0)
        err, e_ex = e.abs().max().item(), ee.abs().max().item()
        rms, rms_ex = e.pow(2).mean().sqrt().item(), ee.pow(2).mean().sqrt().item()
        worst_r = max(worst_r, err / max(e_ex, 1e-300))
        worst_rms = max(worst_rms, rms / max(rms_ex, 1e-300))
        worst_g = max(worst_g, (e.abs() / (gam * A)).max().item())
        assert err <= SPLIT_EXACT_FACTOR * e_ex + SPLIT_SLACK * scale, (p, err, e_ex, scale)
        assert rms <= SPLIT_RMS_FACTOR * rms_ex, (p, rms, rms_ex)
        assert torch.all(e.abs() <= SPLIT_GAMMA * gam * A), (p, worst_g)
    print(f"wino gemm {case} [{inst}] nblk {geo['nblk']} grid {geo['grid']}: worst / exact err {worst_r:.2f}, rms ratio {worst_rms:.2f}, "
          f"worst / gamma_K A {worst_g:.3f}")


# ------------------------------------------------------------------------------------------------ (f): bitwise invariances
def _w_for(ops, mode, Cout, Cin, k, g):
    w = torch.randn(Cout, k[0], k[1], Cin, generator=g, device="cuda") * (2.0 / (k[0] * k[1] * Cin)) ** 0.5
    if mode == "bf16":
        w = w.bfloat16()
    return ops.attach_split(w, False) if mode != "split" else w


LEAN_ROW_CASES = [
    # inst, mode, Cin, Cout, residual
    ("pp<2,4,lean>", "split", 64, 256, False),
    ("pp<4,2,lean>", "split", 96, 384, False),
    ("split<128,lean>", "split", 64, 128, True),
    ("split<64,lean>", "split", 128, 192, False),
    ("f32<128,wide,lean>", "f32", 64, 128, True),
    ("f32<64,wide,lean>", "f32", 32, 64, False),
]


@pytest.mark.parametrize("case", LEAN_ROW_CASES, ids=lambda c: c[0])
def test_lean_row_range_equals_its_own_launch(ops, case, monkeypatch):
    """Rows [r0, r0 + m) of a large lean launch equal a launch over just those rows (input / output / residual pointers offset),
    r0 not tile-aligned among them."""
    monkeypatch.setattr(ops, "SPLIT_MIN_K", 0)
    inst, mode, Cin, Cout, use_res = case
    assert _instance(mode, Cin, Cout, (1, 1), (1, 1), (0, 0), use_res) == inst
    M = 9000
    g = torch.Generator(device="cuda").manual_seed(SEED + Cin + Cout)
    x = torch.randn(1, M, 1, Cin, generator=g, device="cuda")
    w = _w_for(ops, mode, Cout, Cin, (1, 1), g)
    b = torch.randn(Cout, generator=g, device="cuda")
    res = torch.randn(1, M, 1, Cout, generator=g, device="cuda") if use_res else None
    full = ops.conv2d(x, w, b, relu=True, residual=res)
    for r0, m in ((0, 300), (1, 255), (77, 1000), (257, 4097), (M - 130, 130)):
        part = ops.conv2d(x[:, r0:r0 + m], w, b, relu=True, residual=res[:, r0:r0 + m] if use_res else None)
        assert torch.equal(part, full[:, r0:r0 + m]), (inst, r0, m)


IMAGE_CASES = [
    # name, mode, N, H, W, Cin, Cout, k, stride, pad, residual
    ("pp<2,4,gen>", "split", 3, 21, 17, 32, 256, (3, 3), (2, 2), (1, 1), False),
    ("pp<4,2,gen>", "split", 3, 19, 23, 64, 128, (3, 3), (1, 1), (1, 1), False),
    ("split<128,gen>", "split", 3, 14, 11, 32, 128, (2, 2), (2, 2), (0, 0), True),
    ("split<64,gen>", "split", 3, 15, 13, 64, 64, (3, 3), (1, 1), (1, 1), False),
    ("f32<128,wide>", "f32", 3, 13, 11, 32, 128, (3, 3), (1, 1), (1, 1), True),
    ("bf16<64,wide>", "bf16", 3, 12, 9, 64, 192, (3, 3), (2, 2), (1, 1), False),
]


@pytest.mark.parametrize("case", IMAGE_CASES, ids=lambda c: c[0])
def test_general_image_equals_its_own_launch(ops, case, monkeypatch):
    """Image n of an N-image general-loader launch equals a one-image launch of it."""
    monkeypatch.setattr(ops, "SPLIT_MIN_K", 0)
    inst, mode, N, H, W, Cin, Cout, k, stride, pad, use_res = case
    assert _instance(mode, Cin, Cout, k, stride, pad, use_res) == inst
    g = torch.Generator(device="cuda").manual_seed(SEED + H * W)
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    x = torch.randn(N, H, W, Cin, generator=g, device="cuda").to(dt)
    w = _w_for(ops, mode, Cout, Cin, k, g)
    b = torch.randn(Cout, generator=g, device="cuda")
    Ho, Wo = (H + 2 * pad[0] - k[0]) // stride[0] + 1, (W + 2 * pad[1] - k[1]) // stride[1] + 1
    res = torch.randn(N, Ho, Wo, Cout, generator=g, device="cuda").to(dt) if use_res else None
    full = ops.conv2d(x, w, b, stride, pad, True, res)
    for n in range(N):
        one = ops.conv2d(x[n:n + 1], w, b, stride, pad, True, res[n:n + 1] if use_res else None)
        assert torch.equal(one, full[n:n + 1]), (inst, n)


WINO_FORMS = ["2x2", "42", "42s", "44s", "f64", "f64s", "f64s-v1"]


def _wino_setup(ops, form, monkeypatch, N=3, H=10, W=14, pool=False):
    Cin = 64 if form.startswith("f64") else 128
    Cout = 160 if form == "f64s-v1" else 128
    g = torch.Generator(device="cuda").manual_seed(SEED + len(form))
    x, w, b, r = _wino_inputs(("", form, N, H, W, Cin, Cout, True, None if pool else "slice", pool), g)
    wk, tag = _wino_weights(ops, w, "f64s" if form == "f64s-v1" else form, monkeypatch)
    return x, wk, b, r, tag


@pytest.mark.parametrize("form,pool", [(f, False) for f in WINO_FORMS] + [(f, True) for f in WINO_FORMS if f.startswith("f64")])
def test_winograd_split_staged_and_per_image_equal_one_call(ops, form, pool, monkeypatch):
    """For every Winograd form and the fused Cin = 64 kernels (v1 exact, v1 split at Cout % 64 != 0, v2 split): the one-call launch
    equals (1) the staged launches of PROFILE on, (2) the call whose batch is cut by a small WINO_WS_LIMIT, (3) per image, a one-image
    launch.  pool: the fused max-pool (fused forms only)."""
    x, w, b, r, tag = _wino_setup(ops, form, monkeypatch, pool=pool)
    N = x.shape[0]
    one = ops.conv2d(x, w, b, (1, 1), (1, 1), True, r, pool2=pool)
    ops.PROFILE = []
    staged = ops.conv2d(x, w, b, (1, 1), (1, 1), True, r, pool2=pool)
    tags = [t[4][3] for t in ops.PROFILE if t[2] == "conv_gemm"]
    ops.PROFILE = None
    assert tags == [tag], tags
    assert torch.equal(staged, one), form
    from manuscript_ocr_amd import _native as nat
    _, H, W, Cin = x.shape
    d = nat.ConvDesc()
    d.dtype, d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = nat.F32, N, H, W, Cin, H, W, w.shape[0]
    d.KH, d.KW, d.stride_h, d.stride_w, d.pad_h, d.pad_w = 3, 3, 1, 1, 1, 1
    d.in_sN, d.in_sH, d.in_sW, d.out_ld, d.flags = x.stride(0), x.stride(1), x.stride(2), w.shape[0], nat.CONV_POOL2 if pool else 0
    L = nat.lib()
    if form.startswith("f64"):
        full_ws = L.msocr_winograd_fused64_workspace_bytes(ctypes.byref(d))
    else:
        full_ws = L.msocr_winograd_workspace_bytes(ctypes.byref(d), {"2x2": nat.WINO_2X2, "44s": nat.WINO_4X4}.get(form, nat.WINO_4X2))
    assert full_ws > 0
    monkeypatch.setattr(ops, "WINO_WS_LIMIT", full_ws // N + 1)   # one image per part
    for prof in (None, []):
        ops.PROFILE = prof
        cut = ops.conv2d(x, w, b, (1, 1), (1, 1), True, r, pool2=pool)
        ops.PROFILE = None
        assert torch.equal(cut, one), (form, "workspace split", prof is not None)
    monkeypatch.setattr(ops, "WINO_WS_LIMIT", 1 << 30)
    for n in range(N):
        img = ops.conv2d(x[n:n + 1], w, b, (1, 1), (1, 1), True, r[n:n + 1] if r is not None else None, pool2=pool)
        assert torch.equal(img, one[n:n + 1]), (form, n)


EPILOGUE_CASES = [
    # inst, mode, Cin, Cout, k, stride, pad, residual
    ("pp<2,4,lean>", "split", 64, 256, (1, 1), (1, 1), (0, 0), False),
    ("pp<4,2,gen>", "split", 32, 128, (3, 3), (2, 2), (1, 1), False),
    ("split<128,lean>", "split", 64, 128, (1, 1), (1, 1), (0, 0), True),
    ("split<64,gen>", "split", 32, 64, (3, 3), (1, 1), (1, 1), False),
    ("f32<128,wide,lean>", "f32", 64, 128, (1, 1), (1, 1), (0, 0), False),
    ("f32<32,narrow>", "f32", 16, 32, (3, 3), (1, 1), (1, 1), True),
    ("bf16<128,narrow>", "bf16", 32, 128, (3, 3), (1, 1), (1, 1), False),
    ("wino:42s", "wino", 128, 128, (3, 3), (1, 1), (1, 1), False),
    ("wino:f64s", "wino", 64, 128, (3, 3), (1, 1), (1, 1), False),
]


@pytest.mark.parametrize("case", EPILOGUE_CASES, ids=lambda c: c[0])
def test_no_bias_and_relu_epilogues(ops, case, monkeypatch):
    """bias=None equals bias=zeros (the pp producers then read msocr_pp_zero16), and relu=True equals relu=False clamped at 0."""
    monkeypatch.setattr(ops, "SPLIT_MIN_K", 0)
    inst, mode, Cin, Cout, k, stride, pad, use_res = case
    g = torch.Generator(device="cuda").manual_seed(SEED + Cin * Cout)
    N, H, W = 2, 11, 13
    if mode == "wino":
        x, w, b, r, tag = _wino_setup(ops, inst[5:], monkeypatch, N, H, W)
        res = r if use_res else None
    else:
        assert _instance(mode, Cin, Cout, k, stride, pad, use_res) == inst
        dt = torch.bfloat16 if mode == "bf16" else torch.float32
        x = torch.randn(N, H, W, Cin, generator=g, device="cuda").to(dt)
        w = _w_for(ops, mode, Cout, Cin, k, g)
        Ho, Wo = (H + 2 * pad[0] - k[0]) // stride[0] + 1, (W + 2 * pad[1] - k[1]) // stride[1] + 1
        res = torch.randn(N, Ho, Wo, Cout, generator=g, device="cuda").to(dt) if use_res else None
        b = torch.randn(Cout, generator=g, device="cuda")
    nob = ops.conv2d(x, w, None, stride, pad, False, res)
    zb = ops.conv2d(x, w, torch.zeros_like(b), stride, pad, False, res)
    assert torch.equal(nob, zb), inst
    lin = ops.conv2d(x, w, b, stride, pad, False, res)
    rl = ops.conv2d(x, w, b, stride, pad, True, res)
    assert torch.equal(rl, lin.clamp_min(0)), inst
    assert (lin < 0).any() and (rl == 0).any()


def test_conv2d_split_input_above_2_gb_is_cut_into_image_ranges(ops, monkeypatch):
    """msocr_conv2d_split (pp<4,2,gen>: 3x3 / 2, Cin 64 -> Cout 128) on an input of 3 x 750 MB = 2.25 GB: the entry point launches image
    ranges of 2 + 1 images.  Sampled rows of every image against f64, and each image equal to its own one-image launch."""
    N, H, W, Cin, Cout = 3, 1712, 1712, 64, 128
    img_bytes = H * W * Cin * 4
    per = (2 ** 31 - 1) // img_bytes
    assert N * img_bytes >= 2 ** 31 and 1 <= per < N
    assert _instance("split", Cin, Cout, (3, 3), (2, 2), (1, 1), False) == "pp<4,2,gen>"
    g = torch.Generator(device="cuda").manual_seed(SEED + 2)
    x = torch.randn(N, H, W, Cin, generator=g, device="cuda")
    w = torch.randn(Cout, 3, 3, Cin, generator=g, device="cuda") * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g, device="cuda") * 0.5
    monkeypatch.setattr(ops, "SPLIT_MIN_K", 0)
    monkeypatch.setattr(ops, "SPLIT_BF16X3", 1)
    ops.PROFILE = []
    out = ops.conv2d(x, w, b, (2, 2), (1, 1), True)
    tags = [t[4][3] for t in ops.PROFILE]
    ops.PROFILE = None
    assert tags == ["direct_split"], tags
    Ho, Wo = out.shape[1:3]
    M1 = Ho * Wo
    gc = torch.Generator().manual_seed(SEED)
    rows = torch.cat([torch.randint(0, M1, (700,), generator=gc) + n * M1 for n in range(N)] +
                     [torch.arange(M1 - 64, M1 + 64), torch.arange(2 * M1 - 64, 2 * M1 + 64), torch.arange(N * M1 - 64, N * M1)])
    ref, A, _ = _reference(x, w, b, None, True, rows, Ho, Wo, (2, 2), (1, 1))
    e = (_rows_of(out, rows, Ho, Wo) - ref).abs()
    worst = (e / (SPLIT_GAMMA * _gamma(9 * Cin) * A)).max().item()
    print(f"image-range cut: {N} images of {img_bytes / 1e6:.0f} MB, {per} per launch; err {e.max().item() / ref.abs().max().item():.2e}, "
          f"worst / (SPLIT_GAMMA gamma_K A) {worst:.4f}")
    assert worst <= 1.0
    for n in range(N):
        one = ops.conv2d(x[n:n + 1], w, b, (2, 2), (1, 1), True)
        assert torch.equal(one, out[n:n + 1]), n
        del one
    del x, out
    torch.cuda.empty_cache()
