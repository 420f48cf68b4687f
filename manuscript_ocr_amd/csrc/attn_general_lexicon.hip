// attn_general_lexicon.hip — the general decode kernel (attn_general.hip) compiled as the lexicon-constrained beam decode: the beam
// instantiation alone, with a trie node per slot and the allowed-token mask, behind msocr_internal_attn_general_lexicon
// (msocr_attn_beam_lexicon).  A translation unit of its own, so that the plain kernels' code objects stay as they are; see the comment
// on MSOCR_ATTN_LEXICON there.
#define MSOCR_ATTN_LEXICON 1
#include "attn_general.hip"
