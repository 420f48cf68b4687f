// attn_lm_mfma.hip — the beam decode with a character n-gram language model fused in, on the matrix cores: attn_beam_mfma_kernel of
// attn_beam_mfma.hip with a table row per beam slot and the addend lm_weight * table[ctx][v], with the attention-weight store on, and
// its launcher msocr_internal_attn_lm_mfma, behind msocr_attn_beam_lm_hoisted of trba_kernels.hip.  A translation unit of its own so that
// the code objects of the plain kernels stay what they were (see the notes on ALPHA and MSOCR_ATTN_LM in attn_beam_mfma.hip); no greedy
// kernel, no forced kernel and no pack helpers are compiled here.
#define MSOCR_ATTN_LM 1
#define MSOCR_ATTN_ALPHA 1
#include "attn_beam_mfma.hip"
