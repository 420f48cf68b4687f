// attn_lexicon_mfma.hip — the lexicon-constrained beam decode on the matrix cores: attn_beam_mfma_kernel of attn_beam_mfma.hip with a
// trie node per beam slot and the allowed-token mask, with the attention-weight store on, and its launcher
// msocr_internal_attn_lexicon_mfma, behind msocr_attn_beam_lexicon_hoisted of trba_kernels.hip.  A translation unit of its own so that the
// code objects of the plain kernels stay what they were (see the notes on ALPHA and MSOCR_ATTN_LEXICON in attn_beam_mfma.hip); no
// greedy kernel, no forced kernel and no pack helpers are compiled here.
#define MSOCR_ATTN_LEXICON 1
#define MSOCR_ATTN_ALPHA 1
#include "attn_beam_mfma.hip"
