"""Generates tests/golden/trba_forced.npz: the reference's teacher-forced pass and target packing, as data.

Runs only where the reference sources are present (not collected by pytest, not needed by any test).  It loads the reference's
recognizers/_trba/model/model.py and data/transforms.py through the stubs of _refload.py and records

  * Attention.forward(is_train=True) (model.py:287-320) of a seeded Attention in eval() with sampling_prob 0: its weights, a seeded
    encoder output batch_H, a batch of texts, their packed inputs and the logits it returns (H 64, V 40, T 7, max_len 6, B 5,
    blank id 3);
  * pack_attention_targets (data/transforms.py:123-157) over a dozen strings: empty, exactly max_len, longer, with characters
    outside the charset and with <BLANK>'s character.

    python tests/golden/gen_forced_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload  # noqa: E402

H, V, T, MAX_LEN, B = 64, 40, 7, 6, 5
SEED = 20261019
# <PAD> <SOS> <EOS> <BLANK>, then 36 symbols; "_" is a second name of <BLANK>'s id, so that a text can hold <BLANK>'s character
ITOS = ["<PAD>", "<SOS>", "<EOS>", "<BLANK>"] + list("abcdefghijklmnopqrstuvwxyz0123456789")
ALIAS = {"_": 3}
DECODE_TEXTS = ["abc", "", "z9y8x7", "hello", "q"]
PACK_TEXTS = ["", "a", "abcdef", "abcdefg", "abcdefghijkl", "a_b", "___", "a!b", "!?", "ab cd", "Zebra9", "x_y!z0123", "0123456789"]


def main():
    assert len(ITOS) == V
    stoi = {s: i for i, s in enumerate(ITOS)}
    stoi.update(ALIAS)
    model = _refload.ref_trba_model()
    _refload._install_pkg_stubs()
    _refload._pkg("ref_trba_data", None)
    tr = _refload._load_into("ref_trba_data", "transforms", "recognizers/_trba/data/transforms.py")

    torch.manual_seed(SEED)
    att = model.Attention(H, H, V, stoi["<SOS>"], stoi["<EOS>"], stoi["<PAD>"], stoi["<BLANK>"])
    with torch.no_grad():
        for p in att.parameters():  # default init is U(+-1/8): scaled up so that the logits depend on the tokens fed
            p.mul_(3.0)
    att.eval()
    assert att.sampling_prob == 0.0
    g = torch.Generator().manual_seed(SEED + 1)
    batch_H = torch.randn(B, T, H, generator=g) * 1.4
    text_in, target_y, lengths = tr.pack_attention_targets(DECODE_TEXTS, stoi, MAX_LEN)
    with torch.no_grad():
        logits = att(batch_H, text=text_in, is_train=True, batch_max_length=MAX_LEN)
    assert logits.shape == (B, MAX_LEN + 1, V)
    p_in, p_tgt, p_len = tr.pack_attention_targets(PACK_TEXTS, stoi, MAX_LEN)

    out = {f"w.{k}": v.detach().numpy() for k, v in att.state_dict().items()}
    out.update(
        dims=np.array([H, V, T, MAX_LEN, B], dtype=np.int64),
        stoi_keys=np.array(list(stoi.keys())), stoi_vals=np.array(list(stoi.values()), dtype=np.int64),
        batch_H=batch_H.numpy(), decode_texts=np.array(DECODE_TEXTS), text_in=text_in.numpy(), target_y=target_y.numpy(),
        lengths=lengths.numpy(), logits=logits.numpy(),
        pack_texts=np.array(PACK_TEXTS), pack_text_in=p_in.numpy(), pack_target_y=p_tgt.numpy(), pack_lengths=p_len.numpy())
    path = os.path.join(HERE, "trba_forced.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; logits range", float(logits[..., :3].min()), float(logits.max()))


if __name__ == "__main__":
    main()
