// Host check of marl-hideandseek_amd/csrc/hs_solve_order.h (tests/test_solve_order_host.py builds and runs it).
// It restates what phase_dd (hs_k_physics.h) did before the header existed — rank the keys (a << 8) | b of the accepted
// candidates, exchange the batch's bodies lane by lane — with the eight lanes of a world as a loop, and compares.
//   solve_order_check filing   phase_detect files a world's candidates in ascending key order
//   solve_order_check order    k-th set bit == key ranking, every accepted mask over 16 candidates
//   solve_order_check deps     dependency masks of a batch, the order word, the spread pending bits
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "hs_solve_order.h"

using namespace hs;

constexpr int kLanes = 8, kCand = 16, kSlots = 17;
static std::mt19937_64 rng(20241020);
static int pick(int n) { return (int)(rng() % (unsigned long long)n); }
static int code_of(int a, int b) { return a | (b << 5); }

// ---- the ranking phase_dd<true> used: lane q ranks the keys of candidates q and q + 8 among all sixteen and enters
// them at their rank, 4 bits each, into two words
static void rank_order(const int *code, int ndd, unsigned acc, unsigned ord[2]) {
    int key[kCand];
    for (int k = 0; k < kCand; ++k)
        key[k] = (k < ndd && ((acc >> k) & 1u)) ? (((code[k] & 31) << 8) | ((code[k] >> 5) & 63)) : 0x7fffffff;
    ord[0] = ord[1] = 0u;
    for (int k = 0; k < kCand; ++k) {
        if (key[k] == 0x7fffffff) continue;
        int rank = 0;
        for (int j = 0; j < kCand; ++j) rank += key[j] < key[k];
        ord[rank >> 3] |= (unsigned)k << ((rank & 7) * 4);
    }
}

// ---- phase_detect's filing of a world's body pairs: lane l owns slots l, l + 8, l + 16; a slot's candidates are its
// partners ABOVE it, lowest first; places by prefix sums over the lanes, slot group by slot group; the first `cap` are kept
static int file_pairs(const bool hit[kSlots][kSlots], int ns, int cap, int *code) {
    int n = 0;
    for (int jb = 0; jb < 3; ++jb)
        for (int l = 0; l < kLanes; ++l) {
            const int slot = l + jb * kLanes;
            if (slot >= ns) continue;
            for (int j = slot + 1; j < ns; ++j)
                if (hit[slot][j] || hit[j][slot]) { if (n < cap) code[n] = code_of(slot, j); ++n; }
        }
    return std::min(n, cap);
}

static int check_filing() {
    long cases = 0, full = 0;
    for (int trial = 0; trial < 200000; ++trial) {
        const int ns = 13 + pick(5);
        bool hit[kSlots][kSlots] = {};
        const int density = 1 + pick(12);
        for (int a = 0; a < ns; ++a)
            for (int b = a + 1; b < ns; ++b) hit[a][b] = pick(40) < density;
        int code[kCand];
        const int n = file_pairs(hit, ns, kCand, code);
        full += n == kCand;
        for (int k = 0; k + 1 < n; ++k) {
            const int k0 = ((code[k] & 31) << 8) | (code[k] >> 5), k1 = ((code[k + 1] & 31) << 8) | (code[k + 1] >> 5);
            if (!(k0 < k1)) { std::printf("filing: keys do not ascend at %d (ns %d)\n", k, ns); return 1; }
            ++cases;
        }
    }
    if (full < 1000) { std::printf("filing: only %ld full lists\n", full); return 1; }
    std::printf("filing OK: %ld neighbouring candidates ascend, %ld full lists\n", cases, full);
    return 0;
}

// 16 ascending pair codes from the body slots 0 .. ns - 1
static void draw_codes(int ns, int *code) {
    std::vector<int> all;
    for (int a = 0; a < ns; ++a)
        for (int b = a + 1; b < ns; ++b) all.push_back((a << 8) | b);
    std::shuffle(all.begin(), all.end(), rng);
    std::sort(all.begin(), all.begin() + kCand);
    for (int k = 0; k < kCand; ++k) code[k] = code_of(all[k] >> 8, all[k] & 0xff);
}

static int check_order() {
    // (a) kth_set_bit against its definition, every mask and every k
    for (unsigned acc = 0; acc < (1u << kCand); ++acc) {
        int k = 0;
        for (int bit = 0; bit < kCand; ++bit)
            if ((acc >> bit) & 1u) {
                if (kth_set_bit(acc, k) != bit) { std::printf("order: kth_set_bit(%#x, %d) = %d, not %d\n", acc, k, kth_set_bit(acc, k), bit); return 1; }
                ++k;
            }
    }
    // (b) against the key ranking: every mask, on code lists from 16 and 17 slots (the first and the last sixteen pairs
    // of the pair order among them), and on shorter lists (ndd < 16: bits at and beyond ndd are never set)
    long cases = 0;
    for (int list = 0; list < 24; ++list) {
        int code[kCand];
        const int ns = list % 2 ? 17 : 16;
        if (list < 2) {
            int n = 0;
            for (int a = 0; a < ns && n < kCand; ++a) for (int b = a + 1; b < ns && n < kCand; ++b) code[n++] = code_of(a, b);
        } else if (list < 4) {
            int n = kCand;
            for (int a = ns - 2; a >= 0 && n > 0; --a) for (int b = ns - 1; b > a && n > 0; --b) code[--n] = code_of(a, b);
        } else {
            draw_codes(ns, code);
        }
        const int ndd = list % 5 == 4 ? 1 + pick(kCand) : kCand;
        for (unsigned acc = 0; acc < (1u << ndd); ++acc) {
            unsigned ord[2];
            rank_order(code, ndd, acc, ord);
            const int nacc = __builtin_popcount(acc);
            for (int rk = 0; rk < nacc; ++rk) {
                const int was = (int)((ord[rk >> 3] >> ((rk & 7) * 4)) & 15u);
                if (kth_set_bit(acc, rk) != was) { std::printf("order: list %d mask %#x rank %d: %d, ranking gives %d\n", list, acc, rk, kth_set_bit(acc, rk), was); return 1; }
                ++cases;
            }
        }
    }
    std::printf("order OK: %ld (mask, rank) cases equal the key ranking\n", cases);
    return 0;
}

// ---- the dependency masks as phase_dd computed them: the bodies of pair p come from lane 2 p of the world
static unsigned dep_shuffle(const int *ma, const int *mb, int h) {
    unsigned dep = 0u;
    for (int p = 0; p < kOrdBatch - 1; ++p) {
        const int pa = ma[p], pb = mb[p];
        if (p < h && pa >= 0 && (pa == ma[h] || pa == mb[h] || pb == ma[h] || pb == mb[h])) dep |= 1u << p;
    }
    return dep;
}
// ... and from the header, with the codes moved as the DPP row shifts move them inside a row of 16 lanes: lane i gets
// lane i - d of its row, 0 from beyond the row.  `row`: the codes of the 16 lanes, `lane`: the lane asking.
static int shifted(const int *row, int lane, int d) { return lane - d >= 0 ? row[lane - d] : 0; }

static int check_batch(const int *codes, int nvalid, int other, int half, long &cases) {
    // the world sits in half `half` of its row; the other half holds another world whose lanes all carry code `other`
    int row[16], ma[kOrdBatch], mb[kOrdBatch];
    for (int i = 0; i < 16; ++i) row[i] = other;
    for (int h = 0; h < kOrdBatch; ++h) {
        const int c = h < nvalid ? codes[h] : -1;
        row[half * 8 + 2 * h] = row[half * 8 + 2 * h + 1] = c;
        ma[h] = c < 0 ? -1 : (c & 31); mb[h] = c < 0 ? -1 : ((c >> 5) & 63);
    }
    for (int q = 0; q < kLanes; ++q) {
        const int h = q >> 1, lane = half * 8 + q;
        const unsigned want = dep_shuffle(ma, mb, h);
        const unsigned got = batch_dep_mask(h, row[lane], shifted(row, lane, 2), shifted(row, lane, 4), shifted(row, lane, 6));
        if (got != want) { std::printf("deps: lane %d of half %d: %#x, the shuffle form gives %#x\n", q, half, got, want); return 1; }
        // the order word carries candidate and mask to the velocity pass
        for (int batch = 0; batch < kOrdBatches; ++batch) {
            const int cand = (int)(cases % 16);
            const unsigned w = ord_pack(batch, cand, got) | (batch ? ord_pack(batch - 1, 15 - cand, 7u - got) : 0u);
            if (ord_cand(w, batch) != cand || ord_dep(w, batch) != got) { std::printf("deps: order word\n"); return 1; }
            if (batch + 1 < kOrdBatches && ord_cand(w, batch + 1) != -1) { std::printf("deps: empty batch\n"); return 1; }
        }
        ++cases;
    }
    return 0;
}

static int check_deps() {
    // pairs_touch against the four comparisons, every two pairs of the 17 slots
    for (int a = 0; a < kSlots; ++a) for (int b = a + 1; b < kSlots; ++b)
        for (int c = 0; c < kSlots; ++c) for (int d = c + 1; d < kSlots; ++d)
            if (pairs_touch(code_of(a, b), code_of(c, d)) != (a == c || a == d || b == c || b == d)) { std::printf("deps: pairs_touch\n"); return 1; }
    // the spread of the mask against the pending bits of a ballot: bit 2 p of the world's byte is pair p
    for (unsigned dep = 0; dep < 8; ++dep)
        for (unsigned wp = 0; wp < 256; ++wp) {
            unsigned pendPairs = 0u;
            for (int p = 0; p < kOrdBatch; ++p) pendPairs |= ((wp >> (2 * p)) & 1u) << p;
            const unsigned junk = wp | 0xabcdef00u;                  // (the bits of the worlds above ride along)
            if (((dep & pendPairs) == 0u) != ((dep_spread(dep) & junk & 0x55555555u & 0xffu) == 0u)) { std::printf("deps: spread\n"); return 1; }
            if ((wp & 0xaau) == 0u && ((dep & pendPairs) == 0u) != ((dep_spread(dep) & junk) == 0u)) { std::printf("deps: spread, raw ballot\n"); return 1; }
        }
    long cases = 0;
    // every equality pattern four pairs can have: eight labels for at most eight bodies, mapped onto slots that use every
    // bit of both fields; every batch of four pairs of them, 0 .. 4 of them valid, in either half of the row
    static const int slot_of[8] = {0, 3, 5, 8, 10, 13, 15, 16};
    std::vector<int> pairs;
    for (int a = 0; a < 8; ++a) for (int b = a + 1; b < 8; ++b) pairs.push_back(code_of(slot_of[a], slot_of[b]));
    const int np = (int)pairs.size();
    for (int i = 0; i < np; ++i) for (int j = 0; j < np; ++j) for (int k = 0; k < np; ++k) for (int l = 0; l < np; ++l) {
        const int codes[4] = {pairs[i], pairs[j], pairs[k], pairs[l]};
        const int nvalid = (i + j + k + l) % 5, half = (i ^ l) & 1;
        if (check_batch(codes, nvalid, pairs[(j + k) % np], half, cases)) return 1;
    }
    // random batches from all 136 pairs
    for (int t = 0; t < 400000; ++t) {
        int codes[4];
        for (int h = 0; h < 4; ++h) { const int a = pick(kSlots - 1); codes[h] = code_of(a, a + 1 + pick(kSlots - 1 - a)); }
        const int a = pick(kSlots - 1);
        if (check_batch(codes, pick(5), code_of(a, a + 1 + pick(kSlots - 1 - a)), pick(2), cases)) return 1;
    }
    std::printf("deps OK: %ld lanes equal the shuffle form\n", cases);
    return 0;
}

int main(int argc, char **argv) {
    const char *what = argc > 1 ? argv[1] : "";
    if (!std::strcmp(what, "filing")) return check_filing();
    if (!std::strcmp(what, "order")) return check_order();
    if (!std::strcmp(what, "deps")) return check_deps();
    std::printf("usage: solve_order_check filing|order|deps\n");
    return 2;
}
