// attn_general_forced.hip — the forced (teacher-forced) decode for every shape of the envelope: attn_general.hip's greedy kernel once
// more, fed the given tokens (AttnArgs::tok_in) instead of its own arg-max, and its launcher msocr_internal_attn_general_forced, behind
// msocr_attn_forced of trba_kernels.hip.  A translation unit of its own so that the code of the greedy and beam kernels stays what it
// was (see the note on FORCED in attn_general.hip).
#define MSOCR_ATTN_FORCED 1
#include "attn_general.hip"
