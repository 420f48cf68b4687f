"""The JPEG ingest kernels of csrc/jpeg.hip over their envelope, on the device.  The cases are test_jpeg_envelope_cpu.py's, each
chosen for structure only the kernels have (lane packing, scan steps and carries, grid splits and strides, tiles, edge branches);
that file proves on the CPU that every case is what it claims to be and that the host twin accepts every sync case.  The checkers
are the serial host decoder for coefficients (ingest.jpeg_coefficients' decoder), PIL / read_image for pixels and, where named, the
host twin for status and rounds: bit for bit, no tolerances.  Every stream is PIL's encoder's."""
import ctypes

import numpy as np
import pytest

from manuscript_ocr_amd import _native as nat
from manuscript_ocr_amd import ingest
import test_jpeg_envelope_cpu as env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _page(coef, batch, k):
    info, base = batch.infos[k]
    return coef[base: base + int(info.coef_total)]


def _assert_coefficients(coef, batch, datas, what):
    """Every page's slice of the batch's coefficient array == the serial decoder's."""
    for k, d in enumerate(datas):
        assert np.array_equal(_page(coef, batch, k), env.reference(d)[1]), (what, k)


def _pixels(torch, coef_dev, batch, k, orientation=1):
    """The device reconstruction of page k from the device coefficients."""
    from manuscript_ocr_amd import ops
    info, base = batch.infos[k]
    return ingest._reconstruct(info, coef_dev[base:], "cuda", torch, ops, orientation).cpu().numpy()


def _interval_stage(torch, datas, what, pixel_pages=(0,)):
    """The per-interval kernel on the batch: status 0, coefficients, pixels of `pixel_pages` -> the batch."""
    batch = ingest.ScanBatch([env.parsed(d) for d in datas])
    assert batch.n_pages == len(datas), what
    coef_dev, status = ingest.entropy_batch_device(batch)
    assert not status.cpu().numpy().any(), (what, status)
    _assert_coefficients(coef_dev.cpu().numpy(), batch, datas, what)
    for k in pixel_pages:
        assert np.array_equal(_pixels(torch, coef_dev, batch, k), env.pil_rgb(datas[k])), (what, k)
    return batch


def _sync_stage(torch, datas, subseq_bytes, max_rounds, what, pixel_pages=(), twin=True):
    """The self-synchronising stage on the batch: status 0, coefficients; status and rounds == the host twin's."""
    batch = env.sync_batch(datas, subseq_bytes)
    coef_dev, status, rounds = ingest.entropy_sync_batch_device(batch, max_rounds=max_rounds)
    status, rounds = status.cpu().numpy(), rounds.cpu().numpy()
    assert not status.any(), (what, status)
    _assert_coefficients(coef_dev.cpu().numpy(), batch, datas, what)
    if twin:
        _, st, rd = ingest.entropy_sync_batch_host_twin(batch, max_rounds=max_rounds)
        assert np.array_equal(status, st) and np.array_equal(rounds, rd), (what, rounds, rd)
    for k in pixel_pages:
        assert np.array_equal(_pixels(torch, coef_dev, batch, k), env.pil_rgb(datas[k])), (what, k)
    return batch


# ------------------------------------------------------------------------------------------------ 1. lane packing
def test_huffman_kernel_at_every_lane_packing(gpu):
    """Batches of 4096-interval pages sized from the launcher's rule so that jpeg_huffman_kernel runs with 2, 4, 8, 16 and 32
    lanes per wave (1, 2, 4, 8, 16 pages on 256 CUs): threads at and above `lanes` leave after the table-staging barrier."""
    n_cu = gpu.cuda.get_device_properties(0).multi_processor_count
    seen = set()
    for lanes in env.LANE_SET:
        n = env.pages_for_lanes(n_cu, lanes)
        assert n is not None, (n_cu, lanes)
        datas = [env.lane_page(k) for k in range(n)]
        batch = _interval_stage(gpu, datas, f"lanes {lanes}", pixel_pages=(n - 1,))
        assert batch.max_intervals == env.LANE_INTERVALS
        got = env.launch_lanes(n_cu, batch.n_pages, batch.max_intervals)
        print(f"{n_cu} CUs, {n} pages x {batch.max_intervals} intervals: lanes {got}")
        assert got == lanes
        seen.add(got)
    assert seen == {2, 4, 8, 16, 32}


def test_huffman_kernel_ragged_packed_batch(gpu):
    """A packed launch (lanes >= 8) whose pages have 4096, 1024, 9, 26, 4096 and 21 intervals, the three samplings and grey: most
    workgroups of the short pages leave at once, one of each has lanes beyond the page's last interval."""
    n_cu = gpu.cuda.get_device_properties(0).multi_processor_count
    datas = env.ragged_batch_datas(n_cu)
    batch = _interval_stage(gpu, datas, "ragged", pixel_pages=range(len(env.RAGGED_INTERVALS)))
    assert [env.desc_scan(batch, k)[3] for k in range(len(env.RAGGED_INTERVALS))] == env.RAGGED_INTERVALS
    assert env.launch_lanes(n_cu, batch.n_pages, batch.max_intervals) >= 8


# ------------------------------------------------------------------------------------------------ 2. place kernel edges
def test_place_kernel_at_the_edges_of_its_scan_step_and_of_the_grid_split(gpu):
    """nsub = 255 / 256 / 257 (the 256-subsequence split of the round and write kernels) and 2047 / 2048 / 2049 (the place
    kernel's 2048-count step, its carry, P[nsub]) in one batch — the per-page P offset and pages that end inside the grid — and
    the 2049 case alone."""
    datas = env.place_streams()
    batch = _sync_stage(gpu, datas, env.PLACE_SUBSEQ, ingest.SYNC_MAX_ROUNDS, "place", pixel_pages=(2, 5))
    assert batch.page_base[:, 3].tolist() == env.PLACE_NSUB
    alone = _sync_stage(gpu, datas[5:], env.PLACE_SUBSEQ, ingest.SYNC_MAX_ROUNDS, "place 2049 alone", pixel_pages=(0,))
    assert alone.page_base[:, 3].tolist() == [2049]


def test_place_kernel_carries_nonuniform_counts_past_2048(gpu):
    """More than 2048 subsequences whose block counts differ (a serial noise stream at S = 256, one-MCU intervals cut at S = 16):
    a wrong carry or a wrong exclusive sum moves every block behind it."""
    for name, data, S, cap in env.nonuniform_cases():
        batch = _sync_stage(gpu, [data], S, cap, name, pixel_pages=(0,))
        assert int(batch.page_base[0, 3]) > 2048, name


# ------------------------------------------------------------------------------------------------ 3. DC kernel segments
def test_dc_kernel_segments(gpu):
    """seg = 1, 3, 5 and 12 (resets inside a thread's eight elements), 512 / 700 / 1100 / 1400 (inside a step), 2048 (at every step's
    first element), 2200 (a reset in the middle of a later step, carry across steps on both sides), and no restart interval with L =
    2047 / 2048 / 2049 / 5120 (pure carry); grey pages leave two of the three workgroups idle."""
    cases = env.dc_cases()
    datas = [d for _, d, _ in cases]
    batch = _sync_stage(gpu, datas, ingest.SYNC_SUBSEQ_BYTES, ingest.SYNC_MAX_ROUNDS, "dc", pixel_pages=(1, 5, 11))
    for k, (name, _, scan) in enumerate(cases):
        assert env.dc_scan(batch, k) == scan, name


# ------------------------------------------------------------------------------------------------ 4. stale workspace and outputs
def _sync_call(torch, batch, dev, coef, status, rounds, ws, max_rounds):
    from manuscript_ocr_amd import ops
    nat.check(nat.lib().msocr_jpeg_entropy_decode_sync_device(
        dev["bytes"].data_ptr(), dev["descs"].data_ptr(), batch.n_pages, dev["bounds"].data_ptr(), dev["sub"].data_ptr(),
        dev["base"].data_ptr(), batch.max_subseq, batch.total_subseq, batch.subseq_bytes, max_rounds, coef.data_ptr(), batch.coef_total,
        status.data_ptr(), rounds.data_ptr(), ws.data_ptr(), ops._stream()), "jpeg_entropy_decode_sync_device")
    torch.cuda.synchronize()


def test_sync_stage_ignores_stale_workspace_and_outputs(gpu):
    """msocr_jpeg_entropy_decode_sync_device twice into one workspace / coef / status / rounds: first over 0xA5 bytes, then over
    what a different batch left there.  Both results are the serial decoder's; the workspace bytes behind
    msocr_jpeg_sync_workspace_bytes stay as they were."""
    torch = gpu
    cap = ingest.SYNC_MAX_ROUNDS
    a_datas = env.place_streams()
    b_datas = [d for _, d, _ in env.dc_cases()][:6]
    A, B = env.sync_batch(a_datas, env.PLACE_SUBSEQ), env.sync_batch(b_datas, ingest.SYNC_SUBSEQ_BYTES)
    need = {id(b): int(nat.lib().msocr_jpeg_sync_workspace_bytes(b.total_subseq, b.n_pages, cap)) for b in (A, B)}
    assert min(need.values()) > 0
    ws = torch.empty(max(need.values()) + 4096, dtype=torch.uint8, device="cuda")
    coef = torch.empty(max(A.coef_total, B.coef_total), dtype=torch.int16, device="cuda")
    status = torch.empty(max(A.n_pages, B.n_pages), dtype=torch.int32, device="cuda")
    rounds = torch.empty_like(status)
    for t in (ws, coef, status, rounds):
        t.view(torch.uint8).fill_(0xA5)
    dev = {id(b): {"bytes": torch.from_numpy(b.bytes).cuda(), "descs": torch.from_numpy(b.descs).cuda(),
                   "bounds": torch.from_numpy(b.bounds).cuda(), "sub": torch.from_numpy(b.sub_first).cuda(),
                   "base": torch.from_numpy(b.page_base).cuda()} for b in (A, B)}
    twin = {id(b): ingest.entropy_sync_batch_host_twin(b, max_rounds=cap) for b in (A, B)}
    for step, (batch, datas) in enumerate(((A, a_datas), (B, b_datas), (A, a_datas))):
        before = ws.cpu().numpy().copy()
        _sync_call(torch, batch, dev[id(batch)], coef, status, rounds, ws, cap)
        after = ws.cpu().numpy()
        assert np.array_equal(after[need[id(batch)]:], before[need[id(batch)]:]), step
        if step == 0:
            assert (after[need[id(batch)]:] == 0xA5).all()
        assert not status[: batch.n_pages].cpu().numpy().any(), step
        assert np.array_equal(rounds[: batch.n_pages].cpu().numpy(), twin[id(batch)][2]), step
        _assert_coefficients(coef.cpu().numpy(), batch, datas, f"stale step {step}")
        assert not np.array_equal(after, before)


# ------------------------------------------------------------------------------------------------ 5. colour-stage grid stride
@pytest.mark.parametrize("name", ["grey", "420"])
def test_colour_stage_past_its_grid(gpu, tmp_path, name):
    """4099 x 4111 = 16.85 M pixels, above the 65535 x 256 the capped grid of jpeg_color_kernel covers in one pass: the second
    pass of the grid-stride loop writes the last rows upright, and — through the mirrored kernel — the first rows upside down."""
    by_o = env.big_frames()[name]
    info = env.reference(by_o[1])[0]
    assert info.width * info.height > 65535 * 256
    for o in (1, 3):
        got = ingest.decode_jpeg_device(by_o[o])
        exp = env.expected_image(tmp_path, by_o[o])
        assert got is not None and tuple(got.shape) == exp.shape
        assert torch_equal(gpu, got, exp), (name, o)


def torch_equal(torch, got_dev, exp):
    """Exact equality of a device u8 tensor and a host array, compared on the device (50 MB pages)."""
    return bool(torch.equal(got_dev, torch.from_numpy(exp).to(got_dev.device)))


# ------------------------------------------------------------------------------------------------ 6. tile and chroma edges
def _device_decode(data):
    got = ingest.decode_jpeg_device(data)
    return None if got is None else got.cpu().numpy()


def test_tile_and_chroma_edges_upright_420(gpu, tmp_path):
    """All 121 pairs of 1..5, 63..65, 127..129 at 4:2:0: every edge branch of the h2v2 upsampling (two or fewer chroma columns, the
    first and last column on even and odd X, the clamped neighbour row) on both entropy routes."""
    env.check_edge_cases(env.edge_sweep(), _device_decode, tmp_path)


@pytest.mark.parametrize("orientation", range(1, 9))
def test_tile_and_chroma_edges_every_orientation(gpu, tmp_path, orientation):
    """Every size on each axis, per sampling: frames narrower than a wave, one short of / exactly / one past one and two 64-pixel
    tiles, mirrored (2..4) and through the transposing kernel (5..8), on both entropy routes."""
    env.check_edge_cases(env.edge_cover(orientation), _device_decode, tmp_path)


# ------------------------------------------------------------------------------------------------ 7. range ends
def test_range_ends_on_both_entropy_stages(gpu):
    """0 / 255 noise at quality 100 (IDCT output far outside [0, 255]: both clamping branches of idct_range_limit; full blocks, long
    codes and dense 0xFF stuffing in the bit readers) and at quality 1 (quantisers of 255, nearly empty blocks)."""
    cases = env.range_cases()
    both = [d for _, d, interval, _ in cases if interval]
    assert len(both) == 16
    _interval_stage(gpu, both, "range, per-interval", pixel_pages=range(len(both)))
    datas = [d for _, d, _, sync in cases if sync]
    # one batch: rounds are per page, the twin takes the same ones
    _sync_stage(gpu, datas, ingest.SYNC_SUBSEQ_BYTES, env.RANGE_ROUNDS, "range, sync", pixel_pages=range(len(datas)))


# ------------------------------------------------------------------------------------------------ info_ok: the sampling forms
def test_reconstruct_refuses_sampling_forms_no_parse_produces(gpu):
    """h1v2 and 2 x 2 chroma through the public entries: MSOCR_E_ARG, nothing launched, the output as it was filled."""
    torch = gpu
    from manuscript_ocr_amd import ops
    lib = nat.lib()
    for name, info, coef in env.bad_sampling_infos():
        coef_dev = torch.from_numpy(coef).cuda()
        ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
        out = torch.full((32, 32, 3), 0xA5, dtype=torch.uint8, device="cuda")
        assert lib.msocr_jpeg_workspace_bytes(ctypes.byref(info)) == -1, name
        assert lib.msocr_jpeg_reconstruct(ctypes.byref(info), coef_dev.data_ptr(), ws.data_ptr(), out.data_ptr(), ops._stream()) == -1, name
        for o in (1, 3, 6):
            assert lib.msocr_jpeg_reconstruct_oriented(ctypes.byref(info), o, coef_dev.data_ptr(), ws.data_ptr(), out.data_ptr(),
                                                       ops._stream()) == -1, (name, o)
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all()) and not bool(ws.any()), name
