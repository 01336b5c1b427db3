// The routed pack (hs_pack_policy_inputs_routed): k_pack_norm (hs_k_norm.h) for a league or a population.  One launch
// packs every agent row into SLOT order (row_of_slot of hs_league_step), normalises each row with the table of the policy
// that owns the slot, and collects the moments per policy.  Output row s has the bits of row row_of_slot[s] of
// k_pack_norm under tables[s / (R / N)]; the moments of policy p are those of its slots.
//
// The body is pack_blocks (hs_k_pack.h) itself, with its image, its pack_write and its moments.  The grid is (g, policy):
// a workgroup belongs to one policy and hands pack_blocks that policy's view of the arguments: its R / N slots as the
// rows, its part of the outputs, its table, its rows [policy][g] of the workspace [N][G][kPackMoments].  So the blocks are
// cut per policy (R / N need not be a multiple of kPackRows), a block has one table and one moments accumulator, and its
// output rows are one contiguous range.  With one policy that is k_pack's grid, block for block, so the moments have
// k_pack's bits.
// What differs is the staging (PackRouted, pack_blocks' Route): the rows of a block are not one byte range of an export.
// The block's row_of_slot goes to LDS first; then, table by table, lane e takes element e of the [slots][W] piece list,
// i.e. column e % W of slot e / W, from row * W + column of the export: a slot's piece is W x 4 contiguous bytes, 4-byte
// aligned (W is odd for some tables), and the k rows of one side of a world are consecutive rows at consecutive slots, so
// a wave's 64 loads fall into a few contiguous runs.  A slot whose row is outside [0, R) stages zeros (mask 0: nothing for
// the moments), is counted, and its output rows are overwritten with zeros after pack_write (piece for piece by the lane
// that wrote it, so the two stores are in program order), on a path no well-formed routing takes.
// k_partials_sum adds each policy's G workspace rows in its fixed order.  No float atomics: the same inputs give the same
// bits.
//
// Every kernel here is a template, emitted where its launch names it, as hs_k_norm.h explains.
#pragma once
#include "hs_k_norm.h"

namespace hs {

struct PackRoutedArgs {
    PackArgs p;                           // rows = R; partials = the routed workspace [N][G][kPackMoments]
    const int32_t *rowOfSlot;             // [R]
    const float *tables;                  // [N][kNormTable], or null (NORM false)
    int32_t *bad;                         // [1], zeroed before the launch, or null
    int perPolicy;                        // R / N
};

// Workgroups per policy: every policy's blocks, up to a share of k_pack's cap (N * G <= kPackMaxGrid rows of workspace).
__host__ __device__ constexpr int pack_routed_grid(int perPolicy, int numPolicies) {
    const int nb = (perPolicy + kPackRows - 1) / kPackRows, cap = kPackMaxGrid / numPolicies;
    return nb < cap ? nb : cap;
}

// Elements [0, nrows * W) of the block's piece list of a table with W per row, to dst[slot * STRIDE + col] through f();
// a slot without a row gets zeros.
template <int W, int STRIDE, typename T, typename F>
HSD void pack_routed_stage(const T *__restrict__ src, const int32_t *rowOf, int nrows, float *dst, F f) {
    const int n = nrows * W;
    for (int e = threadIdx.x; e < n; e += kPackThreads) {
        const int r = e / W, c = e - r * W;
        const int32_t row = rowOf[r];
        dst[r * STRIDE + c] = row < 0 ? 0.f : f(src[(size_t)row * W + c]);
    }
}

// Zeros over the output rows of the block's slots that have no row: lane q's 16-byte pieces are pack_write's.
template <typename T> HSD void pack_routed_zero(T *out, size_t slot0, int nrows, const int32_t *rowOf) {
    constexpr int kPerRow = kPackRow * (int)sizeof(T) / 16;
    float4 *dst = (float4 *)(out + slot0 * kPackRow);
    for (int q = threadIdx.x; q < nrows * kPerRow; q += kPackThreads)
        if (rowOf[q / kPerRow] < 0) dst[q] = float4{0.f, 0.f, 0.f, 0.f};
}

// pack_blocks' Route of one policy: `a` there is the policy's view (rows = its slots), the exports are still whole.
struct PackRouted {
    const int32_t *rowOfSlot;             // the policy's [R / N]
    int32_t *bad;
    int totalRows;                        // R
    int anyNone;                          // the block in hand has a slot without a row (workgroup-uniform)

    // the row of each slot of the block in hand, -1: none
    HSD static int32_t *rows_of_block() {
        __shared__ int32_t rowOf[kPackRows];
        return rowOf;
    }
    // pack_load's part; called with the previous block's readers done, followed by pack_blocks' barrier
    HSD void load(const PackArgs &a, size_t slot0, int nrows, PackImage &im, bool actor, bool moments) {
        int32_t *rowOf = rows_of_block();
        int none = 0;
        if ((int)threadIdx.x < nrows) {
            int32_t row = rowOfSlot[slot0 + threadIdx.x];
            if (row < 0 || row >= totalRows) { row = -1; none = 1; }
            rowOf[threadIdx.x] = row;
        }
        anyNone = __syncthreads_or(none);
        if (none && bad) atomicAdd(bad, 1);               // an integer count: the order of addition cannot show
        auto same = [](float x) { return x; };
        float *img = im.row;
        pack_routed_stage<1, kPackRow>(a.prep, rowOf, nrows, img, [](int32_t p) { return (float)p / kPackPrepScale; });
        pack_routed_stage<kPackSelfW, kPackRow>(a.selfObs, rowOf, nrows, img + kPackColSelf, same);
        pack_routed_stage<1, kPackRow>(a.selfType, rowOf, nrows, img + kPackColType, [](int32_t t) { return (float)t; });
        pack_routed_stage<kPackLidarW, kPackRow>(a.lidar, rowOf, nrows, img + kPackColLidar, same);
        pack_routed_stage<kPackAgentN * kPackAgentW, kPackRow>(a.agentObs, rowOf, nrows, img + kPackColAgents, same);
        pack_routed_stage<kPackBoxN * kPackBoxW, kPackRow>(a.boxObs, rowOf, nrows, img + kPackColBoxes, same);
        pack_routed_stage<kPackRampN * kPackRampW, kPackRow>(a.rampObs, rowOf, nrows, img + kPackColRamps, same);
        if (actor) {
            pack_routed_stage<kPackAgentN, kPackEntities>(a.visAgents, rowOf, nrows, im.vis, same);
            pack_routed_stage<kPackBoxN, kPackEntities>(a.visBoxes, rowOf, nrows, im.vis + kPackAgentN, same);
            pack_routed_stage<kPackRampN, kPackEntities>(a.visRamps, rowOf, nrows, im.vis + kPackAgentN + kPackBoxN, same);
        }
        if (moments) pack_routed_stage<1, 1>(a.selfMask, rowOf, nrows, im.selfMask, same);
    }
    // after the block's rows are written
    template <typename TA, typename TC> HSD void finish(const PackArgs &a, size_t slot0, int nrows) {
        if (!anyNone) return;
        if constexpr (!std::is_same<TA, PackAbsent>::value) pack_routed_zero((TA *)a.actor, slot0, nrows, rows_of_block());
        if constexpr (!std::is_same<TC, PackAbsent>::value) pack_routed_zero((TC *)a.critic, slot0, nrows, rows_of_block());
    }
};

template <typename TA, typename TC, bool MOM, bool NORM>
__global__ __launch_bounds__(kPackThreads) void k_pack_routed(PackRoutedArgs r) {
    const int policy = blockIdx.y, m = r.perPolicy;
    const size_t slot0 = (size_t)policy * (size_t)m;
    PackArgs a = r.p;                                     // the policy's view
    a.rows = m;
    if constexpr (!std::is_same<TA, PackAbsent>::value) a.actor = (TA *)r.p.actor + slot0 * kPackRow;
    if constexpr (!std::is_same<TC, PackAbsent>::value) a.critic = (TC *)r.p.critic + slot0 * kPackRow;
    if (MOM) a.partials = r.p.partials + (size_t)policy * gridDim.x * kPackMoments;
    const float *table = NORM ? r.tables + (size_t)policy * kNormTable : nullptr;
    pack_blocks<TA, TC, MOM, NORM>(a, table, PackRouted{r.rowOfSlot + slot0, r.bad, r.p.rows, 0});
}

}  // namespace hs
