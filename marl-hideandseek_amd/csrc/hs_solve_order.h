// The pure parts of the body-body solve order (hs_k_physics.h phase_dd): which accepted candidate a pair of lanes takes
// and which earlier manifolds of its batch it has to wait for.  Plain scalar functions like hs_broadphase.h, so that a
// host program can compile them too (tests/host/solve_order_check.cpp).
//
// Order.  The oracle solves a world's body-body manifolds in (a < b) pair order.  phase_detect files the candidates
// ddPair[k] by the lower slot a (slots l of all lanes, then l + 8, l + 16: ascending a), and within a slot by ascending
// partner b (__ffs over a mask of partners above a), so the keys (a, b) ascend with k.  The accepted candidates in
// solve order are therefore the set bits of the accepted mask from the lowest up: no key has to be compared.
//
// Dependencies.  A batch is four manifolds of consecutive ranks, one per pair of lanes (h = 0 .. 3).  Manifold h may
// run once no EARLIER manifold of the batch that is still pending shares a body with it.
#pragma once
#include "hs_core.h"

namespace hs {

constexpr int kOrdBatch = 4;            // manifolds of a world in flight at once (lane pairs of its 8 lanes)
constexpr int kOrdBatches = 4;          // batches a world can have: 16 candidates at most

// place of the k-th set bit (k = 0: the lowest) of a 16-bit mask; k < popcount(mask)
HSD int kth_set_bit(unsigned mask, int k) {
    int pos = 0;
    int c = __builtin_popcount(mask & 0xffu);
    if (k >= c) { k -= c; pos += 8; mask >>= 8; }
    c = __builtin_popcount(mask & 0xfu);
    if (k >= c) { k -= c; pos += 4; mask >>= 4; }
    c = __builtin_popcount(mask & 0x3u);
    if (k >= c) { k -= c; pos += 2; mask >>= 2; }
    c = (int)(mask & 1u);
    if (k >= c) pos += 1;
    return pos;
}

// A pair code is a | b << 5, the low 11 bits of a ddPair entry (a < 32, b < 64); negative = no manifold.
HSD bool pairs_touch(int x, int y) {
    const int xa = x & 31, xb = (x >> 5) & 63, ya = y & 31, yb = (y >> 5) & 63;
    return (xa == ya) | (xa == yb) | (xb == ya) | (xb == yb);
}
// Bit p (p < h) of the result: manifold p of the batch shares a body with manifold h.  `mine`: the code of manifold h;
// prev1, prev2, prev3: the codes of manifolds h - 1, h - 2, h - 3 (whatever they hold where h - d < 0).
HSD unsigned batch_dep_mask(int h, int mine, int prev1, int prev2, int prev3) {
    unsigned dep = 0u;
    if (mine < 0) return dep;
    if (h >= 1 && prev1 >= 0 && pairs_touch(mine, prev1)) dep |= 1u << (h - 1);
    if (h >= 2 && prev2 >= 0 && pairs_touch(mine, prev2)) dep |= 1u << (h - 2);
    if (h >= 3 && prev3 >= 0 && pairs_touch(mine, prev3)) dep |= 1u << (h - 3);
    return dep;
}

// What a lane keeps of its four batches from the position pass to the velocity pass of a substep, a byte per batch:
// candidate index (4 bits), valid (1 bit), dependency mask (3 bits).
HSD unsigned ord_pack(int batch, int cand, unsigned dep) { return ((unsigned)cand | 16u | (dep << 5)) << (8 * batch); }
HSD int ord_cand(unsigned ord, int batch) { const unsigned b = ord >> (8 * batch); return (b & 16u) ? (int)(b & 15u) : -1; }
HSD unsigned ord_dep(unsigned ord, int batch) { return (ord >> (8 * batch + 5)) & 7u; }
// dependency bit p -> bit 2 p: where a ballot over a world's lanes has the pending bit of pair p's first lane
HSD unsigned dep_spread(unsigned dep) { return (dep & 1u) | ((dep & 2u) << 1) | ((dep & 4u) << 2); }

}  // namespace hs
