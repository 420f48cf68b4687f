"""Forced decode, the parts that need no GPU: transforms.pack_targets against the reference's
pack_attention_targets, the teacher-forced replay the GPU tests use as their checker against the reference's own teacher-forced pass
(tests/golden/trba_forced.npz, written by tests/golden/gen_forced_golden.py from the reference's model.py:287-320 and
data/transforms.py:123-157), msocr_seq_logp_host against a float64 log-softmax, and the argument checks of the new entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

from attn_call import attn_decode
from manuscript_ocr_amd import _native as nat
from manuscript_ocr_amd.recognizers._trba.transforms import pack_targets
from test_gpu_seq_f64 import _replay

E_ARG = -1


@pytest.fixture(scope="module")
def gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "trba_forced.npz"))
    g = {k: z[k] for k in z.files}
    g["stoi"] = {str(k): int(v) for k, v in zip(g["stoi_keys"], g["stoi_vals"])}
    return g


# ------------------------------------------------------------------------------------------------ packing
def test_pack_targets_lenient_equals_the_reference(gold):
    max_len = int(gold["dims"][3])
    texts = [str(t) for t in gold["pack_texts"]]
    tok_in, target, trun, packed = pack_targets(texts, gold["stoi"], max_len, strict=False)
    assert tok_in.dtype == target.dtype == trun.dtype == np.int32 and tok_in.shape == target.shape == (len(texts), max_len + 1)
    assert np.array_equal(tok_in, gold["pack_text_in"])
    assert np.array_equal(target, gold["pack_target_y"])
    assert np.array_equal(trun, gold["pack_lengths"])
    # the packed text is what the row stands for: its symbols are the ids in front of EOS
    for t, row, n in zip(packed, target, trun):
        assert [gold["stoi"][c] for c in t] == row[:n - 1].tolist()
    # the fixture holds every case: empty, exactly max_len, longer, unknown characters, <BLANK>'s character
    assert "" in texts and any(len(t) == max_len for t in texts) and any(len(t) > max_len for t in texts)
    assert any("!" in t for t in texts) and any("_" in t for t in texts)


def test_pack_targets_strict_raises_instead_of_narrowing(gold):
    max_len, stoi = int(gold["dims"][3]), gold["stoi"]
    blank = stoi["<BLANK>"]
    for i, t in enumerate(str(t) for t in gold["pack_texts"]):
        unknown = [c for c in t if c not in stoi or stoi[c] == blank]
        if unknown or len(t) > max_len:
            with pytest.raises(ValueError) as e:
                pack_targets(["ab", t], stoi, max_len)  # strict is the default
            assert "texts[1]" in str(e.value) and (repr(unknown[0]) in str(e.value) if unknown else str(len(t)) in str(e.value))
        else:
            strict, lenient = pack_targets([t], stoi, max_len, strict=True), pack_targets([t], stoi, max_len, strict=False)
            assert all(np.array_equal(a, b) for a, b in zip(strict[:3], lenient[:3])) and strict[3] == lenient[3] == [t]
    with pytest.raises(ValueError, match="max_len"):
        pack_targets(["a" * (max_len + 1)], stoi, max_len)
    with pytest.raises(ValueError, match="not in the charset"):
        pack_targets(["a!"], stoi, max_len)
    with pytest.raises(ValueError, match="<BLANK>"):
        pack_targets(["a_"], stoi, max_len)


# ------------------------------------------------------------------------------------------------ the checker of the GPU tests
def test_replay_reproduces_the_reference_teacher_forced_pass(gold):
    """The f32 torch-CPU teacher-forced replay through the oracle's AttentionCell (test_gpu_seq_f64._replay, the checker of
    tests/test_gpu_forced.py) gives the logits of the reference's Attention.forward(is_train=True) bit for bit."""
    from oracle import trba_model as otm
    H, V, T, max_len, B = (int(v) for v in gold["dims"])
    stoi = gold["stoi"]
    att = otm.Attention(H, H, V, stoi["<SOS>"], stoi["<EOS>"], stoi["<PAD>"], stoi["<BLANK>"])
    att.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("w.")}, strict=True)
    att.eval()
    tok_in, target, trun, _ = pack_targets([str(t) for t in gold["decode_texts"]], stoi, max_len)
    assert np.array_equal(tok_in, gold["text_in"]) and np.array_equal(target, gold["target_y"]) and np.array_equal(trun, gold["lengths"])
    got = _replay(att, torch.from_numpy(gold["batch_H"]), torch.from_numpy(gold["text_in"])).numpy()
    assert got.shape == gold["logits"].shape == (B, max_len + 1, V) and got.dtype == np.float32
    assert (got[..., stoi["<BLANK>"]] == np.float32(-1e4)).all()
    assert np.array_equal(got, gold["logits"]), float(np.abs(got - gold["logits"]).max())


# ------------------------------------------------------------------------------------------------ msocr_seq_logp_host
# Per step: a sum of V <= 512 exponentials <= 1 in f32 is off by at most 512 * 2^-24 ~ 3e-5 relative, which is what its logarithm is
# off by absolutely; on top come single ulps of |logit| <= 32 (2e-6 each) from the subtraction of the maximum and of the logarithm.
STEP_ATOL = 1e-4


def _logp_problem(V, B=6, steps=9, temperature=1.0, seed=0):
    rng = np.random.default_rng(seed + V)
    logits = (rng.standard_normal((B, steps, V)) * 6.0).clip(-32, 32).astype(np.float32)
    ids = rng.integers(0, V, (B, steps)).astype(np.int32)
    trun = np.array([steps, 1, 0, steps - 1, 4, steps], dtype=np.int32)[:B]
    x = logits.astype(np.float64)
    if temperature != 1.0:
        x = (logits / np.float32(temperature)).astype(np.float64)  # a true f32 division
    m = x.max(-1, keepdims=True)
    ref = x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))
    ref = np.take_along_axis(ref, ids[..., None].astype(np.int64), -1)[..., 0]
    ref[np.arange(steps)[None, :] >= trun[:, None]] = 0.0
    return logits, ids, trun, ref


def _logp_host(logits, ids, trun, temperature=1.0):
    B, steps, V = logits.shape
    lps, lp = np.full((B, steps), 7.0, dtype=np.float32), np.full(B, 7.0, dtype=np.float32)
    rc = nat.lib().msocr_seq_logp_host(logits.ctypes.data, ids.ctypes.data, trun.ctypes.data, B, V, steps, temperature, lps.ctypes.data,
                                       lp.ctypes.data)
    assert rc == 0
    return lps, lp


@pytest.mark.parametrize("temperature", [1.0, 1.7])
@pytest.mark.parametrize("V", [40, 194, 512])
def test_seq_logp_host_against_f64(V, temperature):
    logits, ids, trun, ref = _logp_problem(V, temperature=temperature)
    steps = logits.shape[1]
    lps, lp = _logp_host(logits, ids, trun, temperature)
    err = np.abs(lps.astype(np.float64) - ref)
    print(f"[forced] seq_logp_host V {V} tau {temperature}: per-step err {err.max():.2e}, row err {np.abs(lp - ref.sum(1)).max():.2e}")
    assert err.max() <= STEP_ATOL
    assert np.abs(lp.astype(np.float64) - ref.sum(1)).max() <= steps * STEP_ATOL
    behind = np.arange(steps)[None, :] >= trun[:, None]
    assert (lps[behind] == 0).all() and lp[trun == 0] == 0
    # the row sum is the f64 sum in step order of the f32 step values, rounded once
    for b in range(len(trun)):
        s = 0.0
        for t in range(trun[b]):
            s += float(lps[b, t])
        assert lp[b] == np.float32(s)


def test_seq_logp_host_flags_an_id_outside_the_charset():
    logits, ids, trun, ref = _logp_problem(194)
    ids[0, 3], ids[3, 0], ids[1, 5] = 194, -1, 1000  # rows 0 and 3 inside t_run; row 1 behind its t_run = 1
    lps, lp = _logp_host(logits, ids, trun)
    assert np.isnan(lps[0, 3]) and np.isnan(lp[0]) and np.isnan(lps[3, 0]) and np.isnan(lp[3])
    ok = np.ones_like(lps, dtype=bool)
    ok[0, 3] = ok[3, 0] = False
    assert np.abs(lps[ok] - ref[ok]).max() <= STEP_ATOL and not np.isnan(lp[[1, 2, 4, 5]]).any() and lps[1, 5] == 0


# ------------------------------------------------------------------------------------------------ C ABI
NEW_SYMBOLS = ("msocr_attn_decode", "msocr_seq_logp", "msocr_seq_logp_host")


def test_library_exports_the_forced_decode():
    L = nat.lib()
    for name in NEW_SYMBOLS:
        assert name in nat.exported_symbols() and hasattr(L, name), name
    header = open(os.path.join(os.path.dirname(nat.__file__), "..", "include", "msocr.h")).read()
    for name in NEW_SYMBOLS:
        assert f" {name}(" in header, name


def _host_args(B=2, T=13, H=256, V=194, steps=26):
    """Host buffers standing in for device memory: the entry points must refuse before they touch any of them."""
    f = lambda *s: np.zeros(s, dtype=np.float32)
    w = nat.AttnWeights()
    keep = [f(H, H), f(H), f(H), f(H, H, 4), f(V, H, 4), f(H, H, 4), f(H, 4), f(H, V), f(V)]
    for name, a in zip(("h2h_wt", "h2h_b", "score_w", "wih_ctx_t", "wih_tok", "whh_t", "b_gates", "gen_wt", "gen_b"), keep):
        setattr(w, name, a.ctypes.data)
    ws = nat.AttnSplitWeights()
    packed = [np.zeros(64, dtype=np.uint16) for _ in range(3)]
    for name, a in zip(("h2h_p", "whh_p", "gen_p"), packed):
        setattr(ws, name, a.ctypes.data)
    bufs = dict(bh=f(B, T, H), ph=f(B, T, H), cg=f(B, T, H, 4), tok=np.ones((B, steps), dtype=np.int32), lg=f(B, steps, V), al=f(B, steps, T))
    return w, ws, bufs, keep + packed


def _forced_rc(hoisted, B=2, T=13, H=256, V=194, steps=26, sos=1, null=None, no_ws=False):
    w, ws, b, _keep = _host_args()
    p = {k: (None if k == null else v) for k, v in b.items()}
    bufs = {"batch_H": p["bh"], "proj_H": p["ph"], "w": None if null == "w" else w, "tok_in": p["tok"], "logits_out": p["lg"],
            "alpha_out": p["al"]}
    if hoisted:  # the matrix-core route: ctx_gates and the split weights
        bufs.update(ctx_gates=p["cg"], ws=None if no_ws else ws)
    return attn_decode(nat.ATTN_FORCED, bufs, B=B, T=T, H=H, V=V, steps=steps, sos_id=sos, blank_id=-1)


def test_forced_entry_points_refuse_bad_arguments_without_a_device():
    for hoisted in (False, True):
        for null in ("bh", "ph", "w", "tok", "lg", "al") + (("cg",) if hoisted else ()):
            assert _forced_rc(hoisted, null=null) == E_ARG, (hoisted, null)
        for bad in (dict(B=0), dict(T=0), dict(T=65), dict(H=32), dict(H=576), dict(H=200), dict(V=0), dict(V=513), dict(steps=0),
                    dict(steps=65), dict(sos=-1), dict(sos=194)):
            assert _forced_rc(hoisted, **bad) == E_ARG, (hoisted, bad)
    # the matrix-core entry point takes its kernel's shapes only, and needs the split weights
    for bad in (dict(H=128), dict(H=320), dict(V=257), dict(T=49), dict(no_ws=True)):
        assert _forced_rc(True, **bad) == E_ARG, bad


# The descriptor itself.  Every call here is refused, so no device is needed: the "good" descriptors are complete but for one later
# argument (sos_id outside the charset), which shows that what comes before it was accepted.
def _desc_rc(mode, extra=(), drop=(), **fields):
    """A complete descriptor of `mode` over host stand-ins (B 2, T 13, H 256, V 194), plus the stand-in buffer `bufs[name]` for every
    field named in `extra`, minus the fields in `drop`."""
    w, _ws, b, _keep = _host_args()
    i32 = np.zeros((2, 26, 8), dtype=np.int32)
    spare = np.zeros(2 * 26 * 8 * 194 + 64, dtype=np.float32)  # 16-byte aligned like every numpy allocation of this size
    assert spare.ctypes.data % 16 == 0
    lex, lm = nat.LexiconArrays(), nat.CharLMTable()
    lex.edge_begin = lex.edge_tok = lex.edge_child = lex.terminal = i32.ctypes.data
    lex.n_nodes, lex.n_edges = 1, 0
    lm.table, lm.order, lm.V, lm.n_ctx = spare.ctypes.data, 1, 194, 1
    pool = {"batch_H": b["bh"], "proj_H": b["ph"], "w": w, "tok_in": b["tok"], "logits_out": b["lg"], "ids_out": i32, "alpha_out": spare,
            "workspace": spare, "fin_step_out": i32, "lexicon": lex, "node_out": i32, "lm": lm, "ctx_out": i32}
    own = {nat.ATTN_GREEDY: ("logits_out", "ids_out"), nat.ATTN_BEAM: ("workspace", "fin_step_out"),
           nat.ATTN_FORCED: ("tok_in", "logits_out", "alpha_out")}.get(mode, ())
    names = [n for n in ("batch_H", "proj_H", "w") + own + tuple(extra) if n not in drop]
    fields = {**dict(B=2, T=13, H=256, V=194, steps=26, beam=8, temperature=1.0, sos_id=1, eos_id=2, blank_id=-1), **fields}
    return attn_decode(mode, {n: pool[n] for n in names}, **fields)


MODES = (nat.ATTN_GREEDY, nat.ATTN_BEAM, nat.ATTN_FORCED)


def test_attn_desc_struct_bytes_and_mode():
    size = ctypes.sizeof(nat.AttnDesc)
    for mode in MODES:
        # the right size is accepted: the call gets as far as the weights, which are missing
        assert _desc_rc(mode, drop=("w",), struct_bytes=size) == E_ARG
        # a wrong one is refused before anything else is read: nothing else in this descriptor is valid either
        for bad in (0, size + 8):
            assert attn_decode(mode, {}, struct_bytes=bad) == E_ARG, (mode, bad)
    for mode in (3, -1):
        assert _desc_rc(mode) == E_ARG, mode
    assert nat.lib().msocr_attn_decode(None, None) == E_ARG


def test_attn_desc_beam_options_need_beam_mode_their_trace_and_the_weight_trace():
    both = ("alpha_out", "lexicon", "node_out", "lm", "ctx_out")
    assert _desc_rc(nat.ATTN_BEAM, extra=both, lm_weight=0.5) == E_ARG                       # a lexicon and a language model together
    for opt, trace in (("lexicon", "node_out"), ("lm", "ctx_out")):
        for mode in (nat.ATTN_GREEDY, nat.ATTN_FORCED):
            assert _desc_rc(mode, extra=(opt,)) == E_ARG, (opt, mode)                           # outside beam mode
            assert _desc_rc(mode, extra=("alpha_out", opt, trace), lm_weight=0.5) == E_ARG, (opt, mode)
        assert _desc_rc(nat.ATTN_BEAM, extra=(opt, trace), lm_weight=0.5) == E_ARG, opt         # without alpha_out
        assert _desc_rc(nat.ATTN_BEAM, extra=("alpha_out", opt), lm_weight=0.5) == E_ARG, opt   # without its own trace
        assert _desc_rc(nat.ATTN_BEAM, extra=("alpha_out", trace)) == E_ARG, opt                # the trace without the option


def test_attn_desc_refuses_a_pointer_its_mode_does_not_read():
    for mode, foreign in ((nat.ATTN_BEAM, "tok_in"), (nat.ATTN_GREEDY, "workspace"), (nat.ATTN_FORCED, "ids_out"),
                          (nat.ATTN_GREEDY, "tok_in"), (nat.ATTN_BEAM, "logits_out"), (nat.ATTN_FORCED, "fin_step_out")):
        assert _desc_rc(mode, extra=(foreign,)) == E_ARG, (mode, foreign)


def test_seq_logp_entry_points_refuse_bad_arguments_without_a_device():
    logits, ids, trun, _ = _logp_problem(40)
    B, steps, V = logits.shape
    lps, lp = np.zeros((B, steps), np.float32), np.zeros(B, np.float32)
    good = [logits.ctypes.data, ids.ctypes.data, trun.ctypes.data, B, V, steps, 1.0, lps.ctypes.data, lp.ctypes.data]
    L = nat.lib()
    assert L.msocr_seq_logp_host(*good) == 0
    for k in (0, 1, 2, 7, 8):
        a = list(good)
        a[k] = None
        assert L.msocr_seq_logp_host(*a) == E_ARG and L.msocr_seq_logp(*a, None) == E_ARG, k
    for k, v in ((3, 0), (4, 0), (4, 513), (5, 0), (5, 65)):
        a = list(good)
        a[k] = v
        assert L.msocr_seq_logp_host(*a) == E_ARG and L.msocr_seq_logp(*a, None) == E_ARG, (k, v)
