// k_observe_half.hip — the bf16 / fp16 instances of K2, the per-call observer
// (k_observe_k2.cuh); vsiq_act_observe_t (k_observe.hip) calls them.
#include "k_observe_k2.cuh"

namespace vsiq {

VSIQ_OBSERVE_INST(bf16_t);
VSIQ_OBSERVE_INST(f16_t);

}  // namespace vsiq
