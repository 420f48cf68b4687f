// attn_forced_mfma.hip — the forced (teacher-forced) decode on the matrix cores: attn_forced_mfma_kernel and its launcher
// msocr_internal_attn_forced_mfma, behind msocr_attn_forced_hoisted of trba_kernels.hip.  The kernel is built from the phase functions of
// attn_beam_mfma.hip with the attention-weight store on; a translation unit of its own so that the code objects of the beam and greedy
// kernels stay what they were (see the note on ALPHA in attn_beam_mfma.hip).
#define MSOCR_ATTN_FORCED 1
#define MSOCR_ATTN_ALPHA 1
#include "attn_beam_mfma.hip"
