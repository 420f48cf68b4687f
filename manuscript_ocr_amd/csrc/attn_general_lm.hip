// attn_general_lm.hip — the general decode kernel (attn_general.hip) compiled as the beam decode with a character n-gram language model
// fused in: the beam instantiation alone, with a table row per slot and the addend where the candidates are formed, behind
// msocr_internal_attn_general_lm (msocr_attn_beam_lm).  A translation unit of its own, so that the plain kernels' code objects stay as
// they are; see the comment on MSOCR_ATTN_LM there.
#define MSOCR_ATTN_LM 1
#include "attn_general.hip"
