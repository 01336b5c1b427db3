// ORACLE — TEST INFRASTRUCTURE ONLY (see hs_ref_math.hpp header).
//
// PARITY UNPINNED: madrona::RNG / madrona::rand (rand::initKey mgr.cpp:678, rand::split_i
// sim.cpp:112,970, RNG::sampleI32 / sampleUniform / randKey — call sites SURVEY §8a-R) are
// not in the reference snapshot.  Chosen generator (documented in DESIGN.md): counter-based
// Threefry-2x32 with 20 rounds (Salmon et al., SC'11), integer-only sampling paths.  RandKey,
// threefry2x32 and RNG are the scalar core's (csrc/hs_core.h), shared with the kernels and pinned
// by known-answer vectors; what follows is the oracle's naming of the two key derivations.
#pragma once
#include "hs_ref_math.hpp"

namespace hsref {

// rand::initKey(seed)  (mgr.cpp:678)
static inline RandKey rand_init_key(uint32_t seed) { return {seed, 0u}; }
// rand::split_i(key, idx, idx_upper)  (sim.cpp:112-113)
static inline RandKey rand_split_i(RandKey k, uint32_t idx, uint32_t idx_upper) {
    return threefry2x32(k, idx, idx_upper);
}

}  // namespace hsref
