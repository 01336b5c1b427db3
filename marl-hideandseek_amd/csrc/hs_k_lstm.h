// The recurrent core after its two gate GEMMs (hs_lstm_cell, hs_lstm_cell_backward): the bias, the four gate
// activations, the cell update, the output gate, the LayerNorm over the H hidden channels and the reset of the carried
// state at an episode's end, what the reference's PolicyRNN (scripts/jax_policy.py, make_policy) does around its LSTM.
// include/hideseek.h states the arithmetic.  The GEMMs stay with the BLAS library: this file starts at their result.
//
// A row moves 4 H gate values and H cell values in and y, h_next and c_next (H each) out, and costs three expf, two
// tanhf and one LayerNorm per channel.
//   lanes     hs_rows.h's StridedMap: lane l holds the channels c = l + 64 q, q < kCh = H / 64 (1, 2, 4 or 8).  A wave
//             takes one row per round and a workgroup of four waves four rows: grid-stride over rounds.  An access of a
//             wave is 64 consecutive elements of one gate's block.
//   params    the 6 kCh values of bias | gamma | beta that a lane needs stay in its registers for the whole kernel.
// The forward uses no LDS and has no barrier.  Nothing in a row's outputs depends on the grid or on the row's position.
//
// The backward recomputes the forward from gates, c_prev, the parameters and clear, writes grad_gates and grad_c_prev of
// its row and keeps the 6 kCh sums of grad_cell_params of its channels in registers over all the rows its wave takes, in
// round order; they leave as the workgroup's slice [blockIdx.x][6 H] of a workspace, as hs_rows.h describes.  A wave
// whose row lies past n adds nothing.  No scratch.
#pragma once
#include "hs_rows.h"

namespace hs {

constexpr int kLstmParamRows = 6;                                       // bias i, f, g, o | gamma | beta, rows of H floats
constexpr int kLstmMaxH = 512;

struct LstmArgs {
    const void *gates;                    // [n][4 H]
    const float *cPrev;                   // [n][H]
    const float *params;                  // [6 H]
    const int *clear;                     // [n], or null
    void *y, *hNext;                      // [n][H], or null
    float *cNext;                         // [n][H], or null
    int n, gatesType, yType;
    float eps;
};

struct LstmBwdArgs {
    const void *gates;
    const float *cPrev;
    const float *params;
    const int *clear;
    const void *gradY;                    // [n][H] of yType
    const void *gradHNext;                // [n][H] of gatesType, or null
    const float *gradCNext;               // [n][H], or null
    void *gradGates;                      // [n][4 H] of gatesType, or null
    float *gradCPrev;                     // [n][H], or null
    float *workspace;                     // [gridDim.x][6 H], or null
    int n, gatesType, yType;
    float eps;
};

HSD float lstm_sigma(float x) { return 1.0f / (1.0f + expf(-x)); }

// What forward and backward both compute of one row, per channel of this lane.
template <int H> struct LstmRow {
    float i[H / 64], f[H / 64], g[H / 64], o[H / 64], cp[H / 64], cn[H / 64], tc[H / 64], h[H / 64], hhat[H / 64];
    float rstd;
};

// P: this lane's parameters [6][kCh] (bias i, f, g, o, gamma, beta)
template <int H>
HSD void lstm_row(const void *gates, int gatesType, const float *cPrev, const float (&P)[kLstmParamRows][H / 64], float eps, int row, int lane,
                  LstmRow<H> &r) {
    constexpr int kCh = H / 64;
    const size_t g0 = (size_t)row * (4 * H), c0 = (size_t)row * H;
    _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
        const int c = lane + 64 * q;
        const float zi = elem_load(gates, gatesType, g0 + c) + P[0][q];
        const float zf = elem_load(gates, gatesType, g0 + H + c) + P[1][q];
        const float zg = elem_load(gates, gatesType, g0 + 2 * H + c) + P[2][q];
        const float zo = elem_load(gates, gatesType, g0 + 3 * H + c) + P[3][q];
        r.cp[q] = cPrev[c0 + c];
        r.i[q] = lstm_sigma(zi); r.f[q] = lstm_sigma(zf); r.g[q] = tanhf(zg); r.o[q] = lstm_sigma(zo);
        r.cn[q] = fmaf(r.f[q], r.cp[q], r.i[q] * r.g[q]);
        r.tc[q] = tanhf(r.cn[q]);
        r.h[q] = r.o[q] * r.tc[q];
    }
    r.rstd = row_norm<kCh>(r.h, eps, r.hhat);
}

template <int H>
__global__ __launch_bounds__(kRowsThreads) void k_lstm_fwd(LstmArgs a) {
    constexpr int kCh = H / 64;
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    float P[kLstmParamRows][kCh];
    lane_params<StridedMap<kCh>>(a.params, lane, P);
    const int nrounds = (a.n + kRowsWaves - 1) / kRowsWaves;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row = round * kRowsWaves + wave;
        if (row >= a.n) break;                                                 // wave-uniform; the later rounds lie further past n
        LstmRow<H> r;
        lstm_row<H>(a.gates, a.gatesType, a.cPrev, P, a.eps, row, lane, r);
        const bool keep = !a.clear || a.clear[row] == 0;
        const size_t c0 = (size_t)row * H;
        _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
            const int c = lane + 64 * q;
            if (a.y) elem_store(a.y, a.yType, c0 + c, fmaf(r.hhat[q], P[4][q], P[5][q]));
            if (a.hNext) elem_store(a.hNext, a.gatesType, c0 + c, keep ? r.h[q] : 0.f);
            if (a.cNext) a.cNext[c0 + c] = keep ? r.cn[q] : 0.f;
        }
    }
}

template <int H>
__global__ __launch_bounds__(kRowsThreads) void k_lstm_bwd(LstmBwdArgs a) {
    constexpr int kCh = H / 64;
    __shared__ float S[kLstmParamRows * H];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    float P[kLstmParamRows][kCh], acc[kLstmParamRows][kCh];
    lane_params<StridedMap<kCh>>(a.params, lane, P);
    _Pragma("unroll") for (int j = 0; j < kLstmParamRows; ++j)
        _Pragma("unroll") for (int q = 0; q < kCh; ++q) acc[j][q] = 0.f;
    const int nrounds = (a.n + kRowsWaves - 1) / kRowsWaves;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row = round * kRowsWaves + wave;
        if (row >= a.n) break;                                                 // wave-uniform; no barrier inside the loop
        LstmRow<H> r;
        lstm_row<H>(a.gates, a.gatesType, a.cPrev, P, a.eps, row, lane, r);
        const bool keep = !a.clear || a.clear[row] == 0;
        const size_t g0 = (size_t)row * (4 * H), c0 = (size_t)row * H;
        float dy[kCh], hb[kCh], dhn[kCh];
        _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
            dy[q] = elem_load(a.gradY, a.yType, c0 + lane + 64 * q);
            hb[q] = P[4][q] * dy[q];
        }
        row_norm_bwd<kCh>(hb, r.hhat, r.rstd, dhn);
        _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
            const int c = lane + 64 * q;
            const float gh = (keep && a.gradHNext) ? elem_load(a.gradHNext, a.gatesType, c0 + c) : 0.f;
            const float gc = (keep && a.gradCNext) ? a.gradCNext[c0 + c] : 0.f;
            const float dh = dhn[q] + gh;
            const float dc = fmaf(dh * r.o[q], 1.0f - r.tc[q] * r.tc[q], gc);
            const float dz[4] = {(dc * r.g[q]) * (r.i[q] * (1.0f - r.i[q])), (dc * r.cp[q]) * (r.f[q] * (1.0f - r.f[q])),
                                 (dc * r.i[q]) * (1.0f - r.g[q] * r.g[q]), (dh * r.tc[q]) * (r.o[q] * (1.0f - r.o[q]))};
            _Pragma("unroll") for (int k = 0; k < 4; ++k) {
                if (a.gradGates) elem_store(a.gradGates, a.gatesType, g0 + k * H + c, dz[k]);
                acc[k][q] = acc[k][q] + dz[k];
            }
            if (a.gradCPrev) a.gradCPrev[c0 + c] = dc * r.f[q];
            acc[4][q] = fmaf(dy[q], r.hhat[q], acc[4][q]);
            acc[5][q] = acc[5][q] + dy[q];
        }
    }
    if (!a.workspace) return;                                                  // uniform over the grid
    wave_sums_to_slice<StridedMap<kCh>>(acc, S, a.workspace + (size_t)blockIdx.x * (kLstmParamRows * H));
}

}  // namespace hs
