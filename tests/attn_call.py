"""The tests' one way to msocr_attn_decode: fill an msocr_attn_desc (nat.AttnDesc) and return the call's code."""
import ctypes

from manuscript_ocr_amd import _native as nat


def _pointer(v):
    """What a pointer field of the descriptor takes: None, an address, a torch tensor, a numpy array or a ctypes struct."""
    if v is None or isinstance(v, int):
        return v
    if isinstance(v, ctypes.Structure):
        return ctypes.pointer(v)
    return v.data_ptr() if hasattr(v, "data_ptr") else v.ctypes.data


def attn_decode(mode, bufs, **fields):
    """mode: nat.ATTN_GREEDY / ATTN_BEAM / ATTN_FORCED.  bufs: descriptor pointer field -> buffer (see _pointer); a field left out stays
    NULL.  fields: the scalar fields (B, T, H, V, steps, beam, sos_id, ...), `stream` for the call's stream (default: the null stream)
    and anything to override, struct_bytes and mode included."""
    stream = fields.pop("stream", None)
    d = nat.AttnDesc(struct_bytes=ctypes.sizeof(nat.AttnDesc), mode=mode)
    for k, v in bufs.items():
        setattr(d, k, _pointer(v))
    for k, v in fields.items():
        setattr(d, k, v)
    return nat.lib().msocr_attn_decode(ctypes.byref(d), stream)
