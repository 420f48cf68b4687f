"""Device-side TRBA network: SE-ResNet31 -> mean over H -> 2 x BiLSTM -> attention decoder.

Host logic only (weight folding / transposition, launch order); arithmetic is in libmsocr.so.
Mirrors /root/reference/src/manuscript/recognizers/_trba/model/model.py:387-416 and
model/seresnet31.py:180-187 with:
  * BatchNorm folded into the bias-free convs (eval mode), NHWC, implicit-GEMM MFMA convs;
  * the 3x3 C=3 stem as a 3-tap conv over a zero-bordered padded-channel canvas;
  * SE gate + residual add + ReLU fused in one kernel per block;
  * LSTM input projections and the Linear layers as MFMA GEMMs (1x1 convs: split-operand bf16x3 with f32 accumulation under
    precision="fp32", exact-f32 MFMA under "fp32-exact"), the recurrence as one persistent launch per layer (both directions);
  * the attention decoder as ONE launch for the whole step loop, i2h(batch_H) hoisted out of it,
    the one-hot matmul replaced by a row gather of W_ih (model.py:36,44: identical arithmetic).
The CNN may run in bf16 (`dtype`).  The recurrent and attention stages keep f32 state and f32 accumulation in every mode; under
precision="fp32" (the default) their matrix products are the split-operand form on the bf16 pipes (f32 result up to summation
order) and their gate nonlinearities use the hardware-rate v_exp_f32 / v_rcp_f32 (1-2 ulp); precision="fp32-exact" runs
exact-f32 MFMA / VALU kernels (the decoder: beam on the matrix-core kernel's exact-f32 form, greedy on the general kernel).
"""
import ctypes

import numpy as np

import torch

from ... import _native as nat
from ... import ops
from ...detectors._east.net import BN_EPS, pack_stem_weight, stem_view, to_khwc


def _fold(sd, conv_key, bn_key):
    w = sd[conv_key + ".weight"].float()
    gamma, beta = sd[bn_key + ".weight"].float(), sd[bn_key + ".bias"].float()
    mean, var = sd[bn_key + ".running_mean"].float(), sd[bn_key + ".running_var"].float()
    s = gamma / torch.sqrt(var + BN_EPS)
    return w * s.view(-1, 1, 1, 1), beta - mean * s


def _gate_interleave(w_t, H):
    """[K, 4H] (columns = gate-major i,f,g,o blocks of H units) -> [K, H, 4]: the 4 gates of unit j adjacent,
    so a lane fetches them with one 16-byte load."""
    K = w_t.shape[0]
    return w_t.reshape(K, 4, H).permute(0, 2, 1).contiguous()


# Decoder entry points: True = the `_hoisted` ones (context half of the LSTMCell input product hoisted out of the step loop) on the
# matrix-core kernels wherever AttnDecoder._matrix_core allows; False = the plain ones, i.e. the general kernel for every shape
# (csrc/attn_general.hip) — what the tests set to cross-check the matrix-core kernels on the device.
HOIST_CTX = True

LAYER_SPEC = (("layer1", 1, 2), ("layer2", 2, 1), ("layer3", 5, 2), ("layer4", 3, 1))


class TrbaNet:
    def __init__(self, state_dict, num_classes, hidden=256, dtype=torch.float32, device="cuda", split=None):
        check_decoder_shape(hidden, num_classes)
        self.dtype, self.device = dtype, torch.device(device)
        self.V, self.Hd = num_classes, hidden
        dev, sd = self.device, state_dict
        P = {}
        self.cpad = 4 if dtype == torch.float32 else 8
        self.cin_pad = 16 if dtype == torch.float32 else 32
        w, b = _fold(sd, "cnn.conv0.0", "cnn.conv0.1")
        P["stem"] = (pack_stem_weight(w, self.cin_pad, self.cpad).to(dtype).to(dev), b.to(dev))
        w, b = _fold(sd, "cnn.conv0.3", "cnn.conv0.4")
        P["conv0b"] = (to_khwc(w, dtype, dev, split), b.to(dev))
        for lname, blocks, stride in LAYER_SPEC:
            for i in range(blocks):
                p = f"cnn.{lname}.{i}."
                for j in (1, 2):
                    w, b = _fold(sd, p + f"conv{j}", p + f"bn{j}")
                    P[f"{lname}.{i}.conv{j}"] = (to_khwc(w, dtype, dev, split), b.to(dev))
                P[f"{lname}.{i}.se"] = (sd[p + "se.fc.0.weight"].float().contiguous().to(dev),
                                        sd[p + "se.fc.2.weight"].float().contiguous().to(dev))
                if p + "downsample.0.weight" in sd:
                    w, b = _fold(sd, p + "downsample.0", p + "downsample.1")
                    P[f"{lname}.{i}.down"] = (to_khwc(w, dtype, dev, split), b.to(dev))
        w, b = _fold(sd, "cnn.conv_out.0", "cnn.conv_out.1")
        P["out0"] = (to_khwc(w, dtype, dev, split), b.to(dev))
        w, b = _fold(sd, "cnn.conv_out.3", "cnn.conv_out.4")
        P["out1"] = (to_khwc(w, dtype, dev, split), b.to(dev))
        self.P = P
        # ---- BiLSTM x2 (f32) ----
        H = hidden
        self.rnn = []
        for l in (0, 1):
            p = f"enc_rnn.{l}."
            w_ih = torch.cat([sd[p + "rnn.weight_ih_l0"], sd[p + "rnn.weight_ih_l0_reverse"]]).float()  # [2*4H, In]
            b = torch.cat([sd[p + "rnn.bias_ih_l0"] + sd[p + "rnn.bias_hh_l0"],
                           sd[p + "rnn.bias_ih_l0_reverse"] + sd[p + "rnn.bias_hh_l0_reverse"]]).float()
            whh_t = torch.stack([_gate_interleave(sd[p + "rnn.weight_hh_l0"].float().t(), H),
                                 _gate_interleave(sd[p + "rnn.weight_hh_l0_reverse"].float().t(), H)])  # [2][H(k)][H(j)][4]
            whh_p = None
            if (ops.SPLIT_BF16X3 if split is None else split) and dtype == torch.float32 and H == 256:
                # W_hh of both directions in the packed split form of the matrix-core recurrence (csrc/bilstm_mfma.hip)
                n = nat.lib().msocr_attn_pack_split_elems(4 * H)
                packed = torch.empty((2, n), dtype=torch.int16)
                wt = whh_t.contiguous()
                for d in (0, 1):
                    nat.check(nat.lib().msocr_attn_pack_split_host(wt[d].data_ptr(), 4 * H, 1, packed[d].data_ptr()), "attn_pack_split_host")
                whh_p = packed.to(dev)
            self.rnn.append({
                "w_ih": w_ih.view(8 * H, 1, 1, -1).contiguous().to(dev), "b": b.contiguous().to(dev),
                "whh_t": whh_t.contiguous().to(dev), "whh_p": whh_p,
                "lin_w": sd[p + "linear.weight"].float().view(H, 1, 1, 2 * H).contiguous().to(dev),
                "lin_b": sd[p + "linear.bias"].float().contiguous().to(dev),
            })
        # ---- attention decoder ----
        self.dec = AttnDecoder(state_dict, num_classes, hidden, split, device,
                               step_split=bool((ops.SPLIT_BF16X3 if split is None else split) and dtype == torch.float32))
        self.att, self._aw, self._asw = self.dec.att, self.dec._aw, self.dec._asw

    # ------------------------------------------------------------------------------------- CNN
    def _se_block(self, x, lname, i, stride):
        P = self.P
        w1, b1 = P[f"{lname}.{i}.conv1"]
        w2, b2 = P[f"{lname}.{i}.conv2"]
        key = f"{lname}.{i}.down"
        idt = ops.conv2d(x, *P[key], stride=(stride, stride)) if key in P else x
        return ops.se_block(x, (w1, b1), (w2, b2), idt, P[f"{lname}.{i}.se"], stride=(stride, stride))

    def cnn(self, canvases_u8):
        """canvases [B,h,w,3] u8 on device (already resized+padded) -> [B,Hf,T,512] NHWC (dtype)."""
        B, h, w, _ = canvases_u8.shape
        x = ops.normalize_u8(canvases_u8, 1, 1, h + 2, w + 4, 1, self.dtype, cpad=self.cpad)
        ws, bs = self.P["stem"]
        x = ops.conv2d(stem_view(x, self.cin_pad), ws, bs, (1, 1), (0, 0), True, out_hw=(h, w), alg_k=27)
        x = ops.conv2d(x, *self.P["conv0b"], pad=(1, 1), relu=True, pool2=True)  # conv0b + ReLU + MaxPool2d(2, 2)
        for lname, blocks, stride in LAYER_SPEC:
            for i in range(blocks):
                x = self._se_block(x, lname, i, stride if i == 0 else 1)
        x = ops.conv2d(x, *self.P["out0"], stride=(2, 1), pad=(0, 1), relu=True)
        return ops.conv2d(x, *self.P["out1"], relu=True)

    # ------------------------------------------------------------------------------------- encoder
    def encode(self, canvases_u8):
        """-> (batch_H [B,T,256] f32, proj_H [B,T,256] f32)."""
        f = self.cnn(canvases_u8)
        B, Hf, T, C = f.shape
        seq = ops.mean_over_h(f)  # [B,T,512] f32
        H = self.Hd
        for l in (0, 1):
            r = self.rnn[l]
            xproj = _gemm(seq.view(B * T, -1), r["w_ih"], r["b"])  # [B*T, 2*4H] = [B][T][2][4H]
            hcat = ops.bilstm_recurrent(xproj, r["whh_t"], B, T, H, r["whh_p"])   # [B,T,2H]
            seq = _gemm(hcat.view(B * T, 2 * H), r["lin_w"], r["lin_b"]).view(B, T, H)
        proj = _gemm(seq.view(B * T, H), self.att["i2h_w"], None).view(B, T, H)
        return seq, proj

    # ------------------------------------------------------------------------------------- decoder
    def greedy(self, batch_H, proj_H, max_len, sos_id, eos_id, blank_id, want_alpha=False):
        return self.dec.greedy(batch_H, proj_H, max_len, sos_id, eos_id, blank_id, want_alpha=want_alpha)

    def forced(self, batch_H, proj_H, tok_in, sos_id, blank_id, ctx_gates=None):
        return self.dec.forced(batch_H, proj_H, tok_in, sos_id, blank_id, ctx_gates=ctx_gates)

    def beam(self, batch_H, proj_H, max_len, beam_size, alpha, temperature, sos_id, eos_id, blank_id, chunks=None, want_alpha=False,
             lexicon=None, lm=None, lm_weight=0.0):
        return self.dec.beam(batch_H, proj_H, max_len, beam_size, alpha, temperature, sos_id, eos_id, blank_id, chunks,
                             want_alpha=want_alpha, lexicon=lexicon, lm=lm, lm_weight=lm_weight)

    def beam_finalize(self, ws, B, steps, beam_size, trun_dev, alpha_ws=None):
        return self.dec.beam_finalize(ws, B, steps, beam_size, trun_dev, alpha_ws=alpha_ws)

    def beam_nbest(self, ws, B, steps, beam_size, trun_dev, n_best, eos_id):
        return self.dec.beam_nbest(ws, B, steps, beam_size, trun_dev, n_best, eos_id)


def check_decoder_shape(hidden, num_classes):
    # hidden_size comes from the checkpoint's config.json (reference __init__.py:142-151, default 256).  256 / <= 256 tokens /
    # beam <= 8 run on the matrix-core decoder kernels (AttnDecoder._matrix_core); other multiples of 64 up to 512, charsets up to
    # 512 tokens and beams up to 16 (beam x hidden <= 4096) on the general one (csrc/attn_general.hip)
    if hidden % 64 or not 64 <= hidden <= 512:
        raise ValueError(f"hidden_size must be a multiple of 64 between 64 and 512 for the HIP recurrent / attention kernels, got {hidden}")
    if num_classes > 512:
        raise ValueError(f"charsets above 512 tokens are not supported by the decoder kernels, got {num_classes}")


def _gemm(x2d, w, b):
    """x2d [M,K] f32 -> [M,N] via the MFMA implicit-GEMM (1x1 conv)."""
    M, K = x2d.shape
    return ops.conv2d(x2d.view(1, M, 1, K), w, b).view(M, w.shape[0])


class AttnDecoder:
    """The attention decoder's device weights (f32, transposed for coalesced column reads) and its launches: greedy, beam,
    beam_finalize, beam_nbest.  Built from the `attn.*` keys of a TRBA state dict; needs no CNN.  split: the hoisted context GEMM's weight
    (ops.attach_split); step_split: pack the split form of the three per-step matrices for the matrix-core kernels (precision
    "fp32" with an f32 CNN — TrbaNet decides)."""

    def __init__(self, state_dict, num_classes, hidden=256, split=None, device="cuda", step_split=None):
        check_decoder_shape(hidden, num_classes)
        if step_split is None:
            step_split = bool(ops.SPLIT_BF16X3 if split is None else split)
        self.device = torch.device(device)
        self.V, self.Hd = num_classes, hidden
        dev, sd, H = self.device, state_dict, hidden
        a = "attn.attention_cell."
        w_ih = sd[a + "rnn.weight_ih"].float()  # [4H, H + V]
        self.att = {
            "i2h_w": sd[a + "i2h.weight"].float().view(H, 1, 1, H).contiguous().to(dev),
            "h2h_wt": sd[a + "h2h.weight"].float().t().contiguous().to(dev),
            "h2h_b": sd[a + "h2h.bias"].float().contiguous().to(dev),
            "score_w": sd[a + "score.weight"].float().view(H).contiguous().to(dev),
            "wih_ctx_t": _gate_interleave(w_ih[:, :H].t(), H).to(dev),
            "wih_tok": _gate_interleave(w_ih[:, H:].t(), H).to(dev),
            "whh_t": _gate_interleave(sd[a + "rnn.weight_hh"].float().t(), H).to(dev),
            "b_gates": _gate_interleave((sd[a + "rnn.bias_ih"] + sd[a + "rnn.bias_hh"]).float().view(1, 4 * H), H).view(H, 4).contiguous().to(dev),
            "gen_wt": sd["attn.generator.weight"].float().t().contiguous().to(dev),
            "gen_b": sd["attn.generator.bias"].float().contiguous().to(dev),
        }
        # rows of rnn.weight_ih[:, :H] reordered unit-major (row j*4+g): the hoisted context product of the beam kernel
        # (msocr_attn_decode with ctx_gates) is one GEMM batch_H x this^T -> [B*T, H*4]
        self.att["wih_ctx_rows"] = ops.attach_split(w_ih[:, :H].reshape(4, H, H).permute(1, 0, 2).reshape(4 * H, 1, 1, H).contiguous().to(dev),
                                                    split)
        aw = nat.AttnWeights()
        for k in ("h2h_wt", "h2h_b", "score_w", "wih_ctx_t", "wih_tok", "whh_t", "b_gates", "gen_wt", "gen_b"):
            setattr(aw, k, self.att[k].data_ptr())
        self._aw = aw
        # split form of the three per-step matrices for the matrix-core beam kernel (precision "fp32"; "fp32-exact" keeps the f32 MFMA)
        self._asw = None
        self._lp_cache = {}  # (alpha, steps) -> the beam's length-penalty table on the device, filled by `beam`
        if step_split and H == 256 and self.V <= 256:
            asw = nat.AttnSplitWeights()
            for src, dst, n, gi in (("h2h_wt", "h2h_p", H, 0), ("whh_t", "whh_p", 4 * H, 1), ("gen_wt", "gen_p", self.V, 0)):
                wt = self.att[src].cpu().contiguous()
                packed = torch.empty((nat.lib().msocr_attn_pack_split_elems(n),), dtype=torch.int16)
                nat.check(nat.lib().msocr_attn_pack_split_host(wt.data_ptr(), n, gi, packed.data_ptr()), "attn_pack_split_host")
                self.att[dst] = packed.to(dev)
                setattr(asw, dst, self.att[dst].data_ptr())
            self._asw = asw

    def _matrix_core(self, T, beam_size=None):
        """Whether a decode of T frames runs on the matrix-core kernels (csrc/attn_beam_mfma.hip: a descriptor with ctx_gates): hidden 256,
        <= 256 tokens, <= 48 frames; greedy also needs the split weights (precision "fp32"), beam a width <= 8 (without the split
        weights it runs on exact-f32 MFMA).  Everything else, and everything under HOIST_CTX = False, runs on the general kernel."""
        if not HOIST_CTX or self.Hd != 256 or self.V > 256 or T > 48:
            return False
        return self._asw is not None if beam_size is None else beam_size <= 8

    def ctx_gates(self, batch_H):
        """W_ih[:, :H] batch_H_t for every frame: [B*T, H*4] (unit-major, gates adjacent), the hoisted context product."""
        B, T, H = batch_H.shape
        return _gemm(batch_H.reshape(B * T, H), self.att["wih_ctx_rows"], None)

    def _desc(self, mode, batch_H, proj_H, steps, sos_id, blank_id, ctx_gates, beam_size=None):
        """A descriptor for msocr_attn_decode with the fields every mode sets.  Where the decode runs on the matrix-core kernels
        (`_matrix_core`) that includes the hoisted context gates, W_ih[:, :H] batch_H_t for every frame once per call instead of
        W_ih[:, :H] ctx in every step (ctx_gates, or computed here), and the split weights if there are any (exact-f32 MFMA without)."""
        B, T, H = batch_H.shape
        d = nat.AttnDesc(struct_bytes=ctypes.sizeof(nat.AttnDesc), mode=mode, B=B, T=T, H=H, V=self.V, steps=steps, sos_id=sos_id,
                         blank_id=-1 if blank_id is None else blank_id, batch_H=batch_H.data_ptr(), proj_H=proj_H.data_ptr(),
                         w=ctypes.pointer(self._aw))
        if self._matrix_core(T, beam_size):
            d.keep = self.ctx_gates(batch_H) if ctx_gates is None else ctx_gates  # alive as long as the descriptor
            d.ctx_gates = d.keep.data_ptr()
            if self._asw is not None:
                d.ws = ctypes.pointer(self._asw)
        return d

    @staticmethod
    def _decode(d, what):
        nat.check(nat.lib().msocr_attn_decode(ctypes.byref(d), ops._stream()), what)

    def greedy(self, batch_H, proj_H, max_len, sos_id, eos_id, blank_id, ctx_gates=None, want_alpha=False, alpha_out=None):
        """ctx_gates: this call's rows of a ctx_gates() result computed beforehand (used only where the kernel takes them).
        want_alpha: also return the attention weights of every step, [B, steps, T] f32 (alpha_out: a buffer of that shape to write
        them to); every other output is the same either way."""
        B, T, H = batch_H.shape
        steps = max_len + 1
        logits = torch.empty((B, steps, self.V), dtype=torch.float32, device=self.device)
        ids = torch.empty((B, steps), dtype=torch.int32, device=self.device)
        al = None
        if want_alpha:
            al = alpha_out if alpha_out is not None else torch.empty((B, steps, T), dtype=torch.float32, device=self.device)
            assert al.shape == (B, steps, T) and al.dtype == torch.float32 and al.is_contiguous() and al.is_cuda
        d = self._desc(nat.ATTN_GREEDY, batch_H, proj_H, steps, sos_id, blank_id, ctx_gates)
        d.eos_id, d.logits_out, d.ids_out = eos_id, logits.data_ptr(), ids.data_ptr()
        if al is not None:
            d.alpha_out = al.data_ptr()
        self._decode(d, "attn_greedy")
        return (logits, ids, al) if want_alpha else (logits, ids)

    def forced(self, batch_H, proj_H, tok_in, sos_id, blank_id, ctx_gates=None):
        """Forced (teacher-forced) decode along given tokens: tok_in [B, steps] int32 on the device, column 0 = SOS, then the ids the
        decoder is to be fed (transforms.pack_targets) -> (logits [B, steps, V] f32, alpha [B, steps, T] f32), every step written.
        Routed like `greedy`; a row fed greedy's own ids gets greedy's logits and weights bit for bit.  ctx_gates as for `greedy`."""
        B, T, H = batch_H.shape
        assert tok_in.dim() == 2 and tok_in.shape[0] == B and tok_in.dtype == torch.int32 and tok_in.is_contiguous() and tok_in.is_cuda
        steps = tok_in.shape[1]
        logits = torch.empty((B, steps, self.V), dtype=torch.float32, device=self.device)
        al = torch.empty((B, steps, T), dtype=torch.float32, device=self.device)
        d = self._desc(nat.ATTN_FORCED, batch_H, proj_H, steps, sos_id, blank_id, ctx_gates)
        d.tok_in, d.logits_out, d.alpha_out = tok_in.data_ptr(), logits.data_ptr(), al.data_ptr()
        self._decode(d, "attn_forced")
        return logits, al

    def seq_logp(self, logits, ids, trun_dev, temperature=1.0):
        """log_softmax(logits / temperature)[ids] per step and summed over t < t_run (msocr_seq_logp): (logp_steps [B, steps] f32,
        logp [B] f32) on the device."""
        B, steps, V = logits.shape
        lps = torch.empty((B, steps), dtype=torch.float32, device=self.device)
        lp = torch.empty((B,), dtype=torch.float32, device=self.device)
        nat.check(nat.lib().msocr_seq_logp(logits.data_ptr(), ids.data_ptr(), trun_dev.data_ptr(), B, V, steps, float(temperature),
                                           lps.data_ptr(), lp.data_ptr(), ops._stream()), "seq_logp")
        return lps, lp

    def beam(self, batch_H, proj_H, max_len, beam_size, alpha, temperature, sos_id, eos_id, blank_id, chunks=None, ctx_gates=None,
             want_alpha=False, alpha_ws=None, lexicon=None, lm=None, lm_weight=0.0):
        """Returns (workspace, fin_step [B] i32, lp) for `beam_finalize`.  ctx_gates as for `greedy`.  Runs all `max_len` steps, or — given
        chunks = (chunk_id [B] i32, chunk_size [nchunks] i32, chunk_state [2*nchunks] i32 zeros), all on the device — only
        as many as the reference's own loop would (it breaks once every beam of the chunk is finished, model.py:215).
        want_alpha: a fourth result, the attention-weight trace [B, steps, beam, T] f32 for `beam_finalize(alpha_ws=...)` (slot-
        indexed like the logits trace; steps the early exit skips stay unwritten); alpha_ws: a buffer of that shape to use.
        lexicon (a recognizers.Lexicon built for this charset and max_len): the search is constrained to the lexicon's words
        (the descriptor's lexicon field) and the result is always (workspace, fin_step, lp, alpha trace,
        nodes): nodes [B, steps, beam] i32, the trie node of every slot after every step (-1 = a dead slot; steps the early exit skips
        stay unwritten).  The workspace is read by beam_finalize / beam_nbest as a plain one is.  None: nothing changes.
        lm (a recognizers.CharLM for this charset and sos_id) with lm_weight (finite, >= 0): every candidate of a live hypothesis gains
        lm_weight * log P_lm(token | context) (the descriptor's lm field) and the result is always
        (workspace, fin_step, lp, alpha trace, ctx): ctx [B, steps, beam] i32, the language model's context of every slot after every
        step (steps the early exit skips stay unwritten).  The workspace holds the model's own logits and is read as a plain one is.
        Not together with a lexicon.  None: nothing changes."""
        B, T, H = batch_H.shape
        steps = max_len
        if lm is not None:
            if lexicon is not None:
                raise ValueError("a language model and a lexicon in one decode are not provided")
            if lm.num_classes != self.V or lm.sos_id != sos_id:
                raise ValueError(f"the language model was built for {lm.num_classes} tokens with sos_id {lm.sos_id}, the decode has "
                                 f"{self.V} tokens and sos_id {sos_id}")
            if not (np.isfinite(lm_weight) and lm_weight >= 0):
                raise ValueError(f"lm_weight must be finite and >= 0, got {lm_weight!r}")
            want_alpha = True
        if lexicon is not None:
            if lexicon.max_len != steps or lexicon.num_classes != self.V:
                raise ValueError(f"the lexicon was built for max_len {lexicon.max_len} and {lexicon.num_classes} tokens, the decode has "
                                 f"{steps} steps and {self.V} tokens")
            want_alpha = True
        nbytes = nat.lib().msocr_attn_beam_workspace_bytes(B, steps, beam_size, self.V)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        fin = torch.empty((B,), dtype=torch.int32, device=self.device)
        lp = None
        if alpha > 0:  # model.py:160, evaluated in Python double then applied in f32; cached: an H2D copy here would make
            #            the host wait for every encoder kernel already queued on this stream
            key = (float(alpha), steps)
            if key not in self._lp_cache:
                self._lp_cache[key] = torch.tensor([((5.0 + (t + 1)) ** alpha) / (6.0 ** alpha) for t in range(steps)],
                                                   dtype=torch.float32).to(self.device)
                torch.cuda.synchronize()
            lp = self._lp_cache[key]
        if not 1 <= beam_size <= 16 or beam_size * H > 4096:
            raise ValueError(f"beam_size {beam_size} with hidden_size {H}: the decoder kernels take beam_size <= 16 and beam_size x hidden_size <= 4096")
        aws = None
        if want_alpha:
            aws = alpha_ws if alpha_ws is not None else torch.empty((B, steps, beam_size, T), dtype=torch.float32, device=self.device)
            assert aws.shape == (B, steps, beam_size, T) and aws.dtype == torch.float32 and aws.is_contiguous() and aws.is_cuda
            assert aws.numel() * 4 == nat.lib().msocr_attn_beam_alpha_bytes(B, steps, beam_size, T)
        d = self._desc(nat.ATTN_BEAM, batch_H, proj_H, steps, sos_id, blank_id, ctx_gates, beam_size)  # the context GEMM is not the decode's
        e = ops._prof_begin()
        d.beam, d.eos_id, d.temperature = beam_size, eos_id, float(temperature)
        d.workspace, d.fin_step_out = ws.data_ptr(), fin.data_ptr()
        if lp is not None:
            d.lp = lp.data_ptr()
        if chunks:
            d.chunk_id, d.chunk_size, d.chunk_state = (c.data_ptr() for c in chunks[:3])
        if aws is not None:
            d.alpha_out = aws.data_ptr()
        if lexicon is not None:  # the constrained kernels: the trie and the node trace
            nodes = torch.empty((B, steps, beam_size), dtype=torch.int32, device=self.device)
            assert nodes.numel() * 4 == nat.lib().msocr_attn_beam_slots_bytes(B, steps, beam_size)
            d.lexicon, d.node_out = lexicon.struct(self.device), nodes.data_ptr()
        elif lm is not None:  # the fused kernels: the table, the weight and the context trace
            ctx_trace = torch.empty((B, steps, beam_size), dtype=torch.int32, device=self.device)
            assert ctx_trace.numel() * 4 == nat.lib().msocr_attn_beam_slots_bytes(B, steps, beam_size)
            d.lm, d.lm_weight, d.ctx_out = lm.struct(self.device), float(lm_weight), ctx_trace.data_ptr()
        self._decode(d, "attn_beam")
        # SURVEY.md 8d, per decode step: proj_H + batch_H (shared by the beams) + LSTMCell W_ih (ctx part + one-hot rows), W_hh,
        # generator, h2h + per row (h, c state + logits); the launch runs up to `steps` of them (chunk-level early exit)
        V, R = self.V, B * beam_size
        per_step = 4.0 * (2 * B * T * H + 4 * H * (H + V) + 4 * H * H + H * V + H * H + R * (4 * H + V))
        ops._prof_end(e, "attn_beam", (per_step, steps), (B, T, beam_size))
        if lexicon is not None:
            return ws, fin, lp, aws, nodes
        if lm is not None:
            return ws, fin, lp, aws, ctx_trace
        return (ws, fin, lp, aws) if want_alpha else (ws, fin, lp)

    def beam_finalize(self, ws, B, steps, beam_size, trun_dev, alpha_ws=None, alpha_out=None):
        """alpha_ws (from `beam(want_alpha=True)`): a third result, the best path's attention weights [B, steps, T] f32, zeros for
        t >= t_run (alpha_out: a buffer of that shape to write them to)."""
        logits = torch.empty((B, steps, self.V), dtype=torch.float32, device=self.device)
        ids = torch.empty((B, steps), dtype=torch.int32, device=self.device)
        al, T = None, 0
        if alpha_ws is not None:
            T = alpha_ws.shape[-1]
            assert alpha_ws.shape == (B, steps, beam_size, T) and alpha_ws.dtype == torch.float32 and alpha_ws.is_contiguous()
            al = alpha_out if alpha_out is not None else torch.empty((B, steps, T), dtype=torch.float32, device=self.device)
            assert al.shape == (B, steps, T) and al.dtype == torch.float32 and al.is_contiguous() and al.is_cuda
        nat.check(nat.lib().msocr_attn_beam_finalize(ws.data_ptr(), B, self.V, steps, beam_size, trun_dev.data_ptr(), logits.data_ptr(),
                                                     ids.data_ptr(), alpha_ws.data_ptr() if al is not None else None, T,
                                                     al.data_ptr() if al is not None else None, ops._stream()), "attn_beam_finalize")
        return (logits, ids) if al is None else (logits, ids, al)
        return logits, ids, al

    def beam_nbest(self, ws, B, steps, beam_size, trun_dev, n_best, eos_id):
        """The `n_best` best final hypotheses of every row, read out of the workspace of `beam` (msocr_attn_beam_nbest; the decode is
        not run again): device tensors ids [B, n_best, steps] i32 (-1 for t >= t_run), prob [B, n_best, steps] f32 (0 there), conf
        [B, n_best] f32 and logp [B, n_best] f32.  Rank 0 is `beam_finalize`'s path with msocr_seq_confidence's confidence, the others
        follow in the search's own order; logp is the summed log-probability up to the hypothesis's first `eos_id`."""
        if not 1 <= n_best <= beam_size:
            raise ValueError(f"n_best must be between 1 and beam_size = {beam_size}, got {n_best}")
        ids = torch.empty((B, n_best, steps), dtype=torch.int32, device=self.device)
        prob = torch.empty((B, n_best, steps), dtype=torch.float32, device=self.device)
        conf = torch.empty((B, n_best), dtype=torch.float32, device=self.device)
        logp = torch.empty((B, n_best), dtype=torch.float32, device=self.device)
        nat.check(nat.lib().msocr_attn_beam_nbest(ws.data_ptr(), B, self.V, steps, beam_size, n_best, eos_id, trun_dev.data_ptr(),
                                                  ids.data_ptr(), prob.data_ptr(), conf.data_ptr(), logp.data_ptr(), ops._stream()),
                  "attn_beam_nbest")
        return ids, prob, conf, logp


def trba_cnn_macs(h, w):
    """Algorithmic MACs of SE-ResNet31 for one h x w crop (2.848 G at 32x100)."""
    macs = h * w * 64 * 27 + h * w * 128 * 64 * 9
    hh, ww, cin = h // 2, w // 2, 128
    for (lname, blocks, stride), planes in zip(LAYER_SPEC, (256, 256, 512, 512)):
        for i in range(blocks):
            s = stride if i == 0 else 1
            h2, w2 = (hh + 2 - 3) // s + 1, (ww + 2 - 3) // s + 1
            macs += h2 * w2 * planes * cin * 9 + h2 * w2 * planes * planes * 9
            if s != 1 or cin != planes:
                macs += h2 * w2 * planes * cin
            macs += 2 * planes * (planes // 16)
            hh, ww, cin = h2, w2, planes
    h3, w3 = (hh - 2) // 2 + 1, (ww + 2 - 2) + 1
    macs += h3 * w3 * 512 * 512 * 4
    macs += (h3 - 1) * (w3 - 1) * 512 * 512 * 4
    return macs
