// attn_beam_mfma_alpha.hip — the matrix-core decode kernels of attn_beam_mfma.hip once more, with the attention weights of every step
// stored (AttnArgs::alpha_out): msocr_internal_attn_beam_mfma_alpha and msocr_internal_attn_greedy_mfma_alpha, behind the _alpha entry
// points of trba_kernels.hip.  A translation unit of its own so that the code object of the plain kernels stays what it was (see the
// note on ALPHA in attn_beam_mfma.hip).
#define MSOCR_ATTN_ALPHA 1
#include "attn_beam_mfma.hip"
