// k_ste_half.hip — the bf16 / fp16 instances of the STE backward (k_ste.cuh), per-tensor
// form; vsiq_act_ste_bwd_t (k_ste.hip) calls them.
#include "k_ste.cuh"

namespace vsiq {

VSIQ_STE_BWD_INST(bf16_t);
VSIQ_STE_BWD_INST(f16_t);

}  // namespace vsiq
