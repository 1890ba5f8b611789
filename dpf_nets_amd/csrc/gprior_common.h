// What gprior.hip (eval), gprior_train.hip and gprior_frozen.hip (the eval-mode backward) share: the canonical block's layout and
// the step codes.  Everything is in an anonymous namespace: each translation unit gets its own copy.
#ifndef DPF_GPRIOR_COMMON_H
#define DPF_GPRIOR_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int MAX_STEPS = 256;

// canon (per step, per net: mu then logvar; the reference's state_dict order, flows.py:176-196):
//   W0 [nf][K] | bn.weight (gamma) | bn.bias (beta) | [bn.running_mean | bn.running_var] | W1 [K][nf] | b1 [K]
// floats of one net: nbn = 4 with the running-statistics slots (dpf_gprior_pack's layout), 2 in the parameters-only layout
__host__ __device__ inline size_t net_floats(int K, int nf, int nbn) { return (size_t)2 * nf * K + (size_t)nbn * nf + K; }

// step code (2 bits): which coordinates a step warps, RealNVPFlowCouple's two patterns (flows.py:224-233)
//   0: even (keep odd)   1: odd (keep even)   2: first half (keep second)   3: second half (keep first)
struct StepCodes { uint32_t w[MAX_STEPS / 16]; };

// n_steps <= MAX_STEPS codes into `packed`, which comes zeroed; false for a code outside 0..3
inline bool pack_step_codes(int n_steps, const int *codes, StepCodes &packed) {
    for (int s = 0; s < n_steps; ++s) {
        if (codes[s] < 0 || codes[s] > 3) return false;
        packed.w[s >> 4] |= (uint32_t)codes[s] << ((s & 15) * 2);
    }
    return true;
}

__device__ __forceinline__ int step_code(const StepCodes &c, int s) { return (c.w[s >> 4] >> ((s & 15) * 2)) & 3; }

// kept coordinate k of a step sits at kmul * k + kadd, warped coordinate i at kmul * i + wadd
struct StepIndex { int kmul, kadd, wadd; };
__host__ __device__ inline StepIndex step_index(int code, int K) {
    return {code < 2 ? 2 : 1, code == 0 ? 1 : code == 2 ? K : 0, code == 1 ? 1 : code == 3 ? K : 0};
}

}  // namespace

#endif
