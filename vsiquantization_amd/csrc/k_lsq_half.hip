// k_lsq_half.hip — the bf16 / fp16 instances of K4 (k_lsq.cuh): the fp32 kernel's body,
// grid, records and fold on 8-byte accesses; vsiq_act_lsq_bwd_t (k_lsq.hip) calls them.
#include "k_lsq.cuh"

namespace vsiq {

VSIQ_LSQ_BWD_INST(bf16_t);
VSIQ_LSQ_BWD_INST(f16_t);

}  // namespace vsiq
