// k_fq_half.hip — the bf16 / fp16 instances of K1 / K5 (k_fq.cuh): the fp32 kernel's
// body, grid and mask layout on 8-byte accesses; vsiq_act_fq_fwd_t (k_fq.hip) calls them.
#include "k_fq.cuh"

namespace vsiq {

VSIQ_FQ_FWD_INST(bf16_t);
VSIQ_FQ_FWD_INST(f16_t);

}  // namespace vsiq
