// k_lsq_half.hip — the bf16 / fp16 instances of K4 and its records-only form K4d
// (k_lsq.cuh): the fp32 kernel's body, grid, records and fold on 8-byte accesses;
// vsiq_act_lsq_bwd_t / vsiq_act_lsq_bwd_part_t (k_lsq.hip) call them.
#include "k_lsq.cuh"

namespace vsiq {

VSIQ_LSQ_BWD_INST(bf16_t);
VSIQ_LSQ_BWD_INST(f16_t);
VSIQ_LSQ_BWD_PART_INST(bf16_t);
VSIQ_LSQ_BWD_PART_INST(f16_t);

}  // namespace vsiq
