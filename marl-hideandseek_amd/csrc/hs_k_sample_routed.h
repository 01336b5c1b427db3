// The routed sampler (hs_sample_actions_routed): k_sample (hs_k_sample.h) for a league or a population.  The logits come
// in SLOT order (row_of_slot of hs_league_step: the P forwards write blocks of one buffer), the actions go out in ROW order,
// where the next step reads them, and what a learner stores (action, log_prob, entropy, head_log_prob) stays in slot order:
// one launch in place of a gather of the logits back to rows, k_sample, and a gather of each stored output to slots.
// For slot s with r = row_of_slot[s], the row-order action of r and every slot-order output at s have the bits k_sample
// gives row r when row r of its logits is slot s's: the head is sample_head itself on the same f32 image, and the uniform
// is keyed by the global agent row worldOffset * A + r, not by the slot, so a draw does not depend on the routing.
//
// The blocks are k_sample's: a workgroup takes kSampleRows consecutive SLOTS, so the logits it reads and the slot-order
// ranges it stores are contiguous, lane for lane as there.  The block's row_of_slot goes to LDS first.  Only the row-order
// store scatters, 4 bytes per (row, head); the k rows of one side of a world are consecutive rows at consecutive slots, so
// a wave's stores fall into runs of 5 k values.  A slot whose row is outside [0, R) is counted in `bad` (an integer
// atomic: the order of addition cannot show), stores zeros to its slot-order outputs and writes no row.  Rows that no slot
// names are not written.  No float atomics, no scratch.
#pragma once
#include "hs_k_sample.h"

namespace hs {

struct SampleRoutedArgs {
    SampleArgs s;                         // logits by slot; action = the row-order actions; logProb, entropy, headLogProb by slot; rows = R
    const int32_t *rowOfSlot;             // [R]
    int32_t *actionSlots;                 // [R][5] by slot, or null
    int32_t *bad;                         // [1], zeroed before the launch, or null
};

template <typename T>
__global__ __launch_bounds__(kSampleThreads) void k_sample_routed(SampleRoutedArgs ra) {
    __shared__ SampleImage im;
    __shared__ int32_t rowOf[kSampleRows];                // the row of each slot of the block in hand, -1: none
    const SampleArgs &a = ra.s;
    const T *logits = (const T *)a.logits;
    const int tid = threadIdx.x, L = a.L, pitch = L | 1;
    const int r = tid / kSampleLanesPerRow, h = tid % kSampleLanesPerRow;
    const int K = h < kSampleHeads ? (int)((a.bucketK >> (8 * h)) & 0xffu) : 0, off = (int)((a.bucketOff >> (8 * h)) & 0xffu);

    const int nblocks = (a.rows + kSampleRows - 1) / kSampleRows;
    for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const int slot0 = b * kSampleRows;
        const int nslots = a.rows - slot0 < kSampleRows ? a.rows - slot0 : kSampleRows;
        if (b != blockIdx.x) __syncthreads();             // the previous block's readers are done with the image
        if (tid < nslots) {
            int32_t row = ra.rowOfSlot[slot0 + tid];
            if (row < 0 || row >= a.rows) {
                row = -1;
                if (ra.bad) atomicAdd(ra.bad, 1);
            }
            rowOf[tid] = row;
        }
        for (int i = tid; i < nslots * L; i += kSampleThreads) {
            const int ri = i / L, c = i - ri * L;
            im.logit[ri * pitch + c] = (float)logits[(size_t)(slot0 + ri) * (size_t)a.stride + c];
        }
        __syncthreads();
        if (r < nslots && h < kSampleHeads) {
            const int q = r * kSampleHeads + h;
            const int32_t row = rowOf[r];
            int act = 0;
            float lp = 0.f, ent = 0.f;
            if (row >= 0) {
                float u = 0.f;
                if (a.mode == kSampleDraw) {
                    const RandKey k = threefry2x32({a.seed0, a.seed1}, a.row0Global + (uint32_t)row, a.counter);
                    RNG rng{k, (uint32_t)h};
                    u = rng.sampleUniform();
                }
                sample_head(im.logit + r * pitch + off, K, a.mode, u, act, lp, ent);
            }
            im.action[q] = act; im.logProb[q] = lp; im.entropy[q] = ent;
        }
        __syncthreads();
        const size_t q0 = (size_t)slot0 * kSampleHeads;
        if (tid < nslots * kSampleHeads) {
            const int32_t row = rowOf[tid / kSampleHeads];
            if (row >= 0) a.action[(size_t)row * kSampleHeads + tid % kSampleHeads] = im.action[tid];
            if (ra.actionSlots) ra.actionSlots[q0 + tid] = im.action[tid];
            if (a.headLogProb) a.headLogProb[q0 + tid] = im.logProb[tid];
        }
        if (tid < nslots) {
            const float *p = im.logProb + tid * kSampleHeads, *e = im.entropy + tid * kSampleHeads;
            if (a.logProb) a.logProb[slot0 + tid] = (((p[0] + p[1]) + p[2]) + p[3]) + p[4];
            if (a.entropy) a.entropy[slot0 + tid] = (((e[0] + e[1]) + e[2]) + e[3]) + e[4];
        }
    }
}

}  // namespace hs
