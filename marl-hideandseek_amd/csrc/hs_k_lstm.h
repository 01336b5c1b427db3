// The recurrent core after its two gate GEMMs (hs_lstm_cell, hs_lstm_cell_backward): the bias, the four gate
// activations, the cell update, the output gate, the LayerNorm over the H hidden channels and the reset of the carried
// state at an episode's end, what the reference's PolicyRNN (scripts/jax_policy.py, make_policy) does around its LSTM.
// include/hideseek.h states the arithmetic.  The GEMMs stay with the BLAS library: this file starts at their result.
//
// A row moves 4 H gate values and H cell values in and y, h_next and c_next (H each) out, and costs three expf, two
// tanhf and one LayerNorm per channel.
//   lanes     k_embed's map with L = 64: lane l holds the channels c = l + 64 q, q < kCh = H / 64 (1, 2, 4 or 8).  A wave
//             takes one row per round and a workgroup of four waves four rows: grid-stride over rounds.  An access of a
//             wave is 64 consecutive elements of one gate's block.
//   params    the 6 kCh values of bias | gamma | beta that a lane needs stay in its registers for the whole kernel.
//   reduce    lstm_sum is emb_sum for these H: ascending q, then the xor butterfly 1, 2, ..., 32.
// The forward uses no LDS and has no barrier.  Nothing in a row's outputs depends on the grid or on the row's position.
//
// The backward recomputes the forward from gates, c_prev, the parameters and clear, writes grad_gates and grad_c_prev of
// its row and keeps the 6 kCh sums of grad_cell_params of its channels in registers over all the rows its wave takes, in
// round order.  The waves then add in LDS as ((w0 + w1) + w2) + w3 and the workgroup writes its slice [blockIdx.x][6 H]
// of a workspace; the grid is capped at kLstmMaxGridBwd, and k_embed_grad_sum (hs_k_embed.h) adds the slices in its fixed
// order.  A wave whose row lies past n adds nothing.  No atomics, no scratch: the same inputs give the same bits.
#pragma once
#include "hs_k_embed.h"                    // emb_load / emb_store, the element types, k_embed_grad_sum

namespace hs {

constexpr int kLstmThreads = 256, kLstmWaves = kLstmThreads / 64;       // a workgroup takes kLstmWaves rows per round
constexpr int kLstmParamRows = 6;                                       // bias i, f, g, o | gamma | beta, rows of H floats
constexpr int kLstmMaxGrid = kEmbMaxGrid;                               // forward
constexpr int kLstmMaxGridBwd = kEmbMaxGridBwd;                         // backward: the slices of the workspace
constexpr int kLstmMaxH = 512;

__host__ __device__ constexpr int lstm_grid(int n, int cap) {
    const int nb = (n + kLstmWaves - 1) / kLstmWaves;
    return nb < cap ? nb : cap;
}

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

// the sum over a row's H channels of p[q] (this lane's channels): ascending q, then the xor butterfly 1, 2, ..., 32
template <int H> HSD float lstm_sum(const float (&p)[H / 64]) {
    float s = p[0];
    _Pragma("unroll") for (int q = 1; q < H / 64; ++q) s = s + p[q];
    _Pragma("unroll") for (int m = 1; m < 64; m <<= 1) s = s + __shfl_xor(s, m, 64);
    return s;
}

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
        const float zi = emb_load(gates, gatesType, g0 + c) + P[0][q];
        const float zf = emb_load(gates, gatesType, g0 + H + c) + P[1][q];
        const float zg = emb_load(gates, gatesType, g0 + 2 * H + c) + P[2][q];
        const float zo = emb_load(gates, gatesType, g0 + 3 * H + c) + P[3][q];
        r.cp[q] = cPrev[c0 + c];
        r.i[q] = lstm_sigma(zi); r.f[q] = lstm_sigma(zf); r.g[q] = tanhf(zg); r.o[q] = lstm_sigma(zo);
        r.cn[q] = fmaf(r.f[q], r.cp[q], r.i[q] * r.g[q]);
        r.tc[q] = tanhf(r.cn[q]);
        r.h[q] = r.o[q] * r.tc[q];
    }
    const float mu = lstm_sum<H>(r.h) / (float)H;
    float d[kCh], dd[kCh];
    _Pragma("unroll") for (int q = 0; q < kCh; ++q) { d[q] = r.h[q] - mu; dd[q] = d[q] * d[q]; }
    const float var = lstm_sum<H>(dd) / (float)H;
    r.rstd = 1.0f / sqrtf(var + eps);
    _Pragma("unroll") for (int q = 0; q < kCh; ++q) r.hhat[q] = d[q] * r.rstd;
}

template <int H> HSD void lstm_params(const float *params, int lane, float (&P)[kLstmParamRows][H / 64]) {
    _Pragma("unroll") for (int j = 0; j < kLstmParamRows; ++j)
        _Pragma("unroll") for (int q = 0; q < H / 64; ++q) P[j][q] = params[j * H + lane + 64 * q];
}

template <int H>
__global__ __launch_bounds__(kLstmThreads) void k_lstm_fwd(LstmArgs a) {
    constexpr int kCh = H / 64;
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    float P[kLstmParamRows][kCh];
    lstm_params<H>(a.params, lane, P);
    const int nrounds = (a.n + kLstmWaves - 1) / kLstmWaves;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row = round * kLstmWaves + wave;
        if (row >= a.n) break;                                                 // wave-uniform; the later rounds lie further past n
        LstmRow<H> r;
        lstm_row<H>(a.gates, a.gatesType, a.cPrev, P, a.eps, row, lane, r);
        const bool keep = !a.clear || a.clear[row] == 0;
        const size_t c0 = (size_t)row * H;
        _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
            const int c = lane + 64 * q;
            if (a.y) emb_store(a.y, a.yType, c0 + c, fmaf(r.hhat[q], P[4][q], P[5][q]));
            if (a.hNext) emb_store(a.hNext, a.gatesType, c0 + c, keep ? r.h[q] : 0.f);
            if (a.cNext) a.cNext[c0 + c] = keep ? r.cn[q] : 0.f;
        }
    }
}

template <int H>
__global__ __launch_bounds__(kLstmThreads) void k_lstm_bwd(LstmBwdArgs a) {
    constexpr int kCh = H / 64;
    __shared__ float S[kLstmParamRows * H];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    float P[kLstmParamRows][kCh], acc[kLstmParamRows][kCh];
    lstm_params<H>(a.params, lane, P);
    _Pragma("unroll") for (int j = 0; j < kLstmParamRows; ++j)
        _Pragma("unroll") for (int q = 0; q < kCh; ++q) acc[j][q] = 0.f;
    const int nrounds = (a.n + kLstmWaves - 1) / kLstmWaves;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row = round * kLstmWaves + wave;
        if (row >= a.n) break;                                                 // wave-uniform; no barrier inside the loop
        LstmRow<H> r;
        lstm_row<H>(a.gates, a.gatesType, a.cPrev, P, a.eps, row, lane, r);
        const bool keep = !a.clear || a.clear[row] == 0;
        const size_t g0 = (size_t)row * (4 * H), c0 = (size_t)row * H;
        float dy[kCh], hb[kCh], hz[kCh];
        _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
            dy[q] = emb_load(a.gradY, a.yType, c0 + lane + 64 * q);
            hb[q] = P[4][q] * dy[q];
            hz[q] = hb[q] * r.hhat[q];
        }
        const float mh = lstm_sum<H>(hb) / (float)H, mhz = lstm_sum<H>(hz) / (float)H;
        _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
            const int c = lane + 64 * q;
            const float gh = (keep && a.gradHNext) ? emb_load(a.gradHNext, a.gatesType, c0 + c) : 0.f;
            const float gc = (keep && a.gradCNext) ? a.gradCNext[c0 + c] : 0.f;
            const float dh = r.rstd * ((hb[q] - mh) - r.hhat[q] * mhz) + gh;
            const float dc = fmaf(dh * r.o[q], 1.0f - r.tc[q] * r.tc[q], gc);
            const float dz[4] = {(dc * r.g[q]) * (r.i[q] * (1.0f - r.i[q])), (dc * r.cp[q]) * (r.f[q] * (1.0f - r.f[q])),
                                 (dc * r.i[q]) * (1.0f - r.g[q] * r.g[q]), (dh * r.tc[q]) * (r.o[q] * (1.0f - r.o[q]))};
            _Pragma("unroll") for (int k = 0; k < 4; ++k) {
                if (a.gradGates) emb_store(a.gradGates, a.gatesType, g0 + k * H + c, dz[k]);
                acc[k][q] = acc[k][q] + dz[k];
            }
            if (a.gradCPrev) a.gradCPrev[c0 + c] = dc * r.f[q];
            acc[4][q] = fmaf(dy[q], r.hhat[q], acc[4][q]);
            acc[5][q] = acc[5][q] + dy[q];
        }
    }
    if (!a.workspace) return;                                                  // uniform over the grid
    for (int w = 0; w < kLstmWaves; ++w) {                                     // ((w0 + w1) + w2) + w3
        if (w) __syncthreads();
        if (wave == w) {
            _Pragma("unroll") for (int j = 0; j < kLstmParamRows; ++j)
                _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
                    const int i = j * H + lane + 64 * q;
                    S[i] = w == 0 ? acc[j][q] : S[i] + acc[j][q];
                }
        }
    }
    __syncthreads();
    float *out = a.workspace + (size_t)blockIdx.x * (kLstmParamRows * H);
    for (int i = threadIdx.x; i < kLstmParamRows * H; i += kLstmThreads) out[i] = S[i];
}

}  // namespace hs
