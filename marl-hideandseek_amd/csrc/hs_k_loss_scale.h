// The dynamic loss scale of float16 training (hs_ppo_loss_scaled, hs_twohot_value_scaled, hs_adam_step_scaled): a scale S
// that lives on the device, which the two loss kernels multiply their gradients by and the optimiser divides out again,
// halving it when the gradient norm overflows and doubling it after a run of good steps (the published rule of
// torch.cuda.amp.GradScaler and flax's DynamicScale; madrona_learn is on no machine, so the rule is this project's).
// include/hideseek.h states the arithmetic.  Nothing here reads the device from the host: the update loop stays free of
// synchronisation.
//
// The state, f64 [kLossScaleState]: S, the good steps since S last changed, the backoffs and the growths so far.
//   k_ppo_scaled, k_twohot_scaled   the unscaled kernels' work (ppo_samples, twohot_samples) with grad_scale * S, the
//                 product in f32, where they have grad_scale; S = (float)state[0] is one uniform load.  The state is read,
//                 never written, and the statistics hold no S.
//   k_adam_norm_scaled   k_adam_norm's partials (adam_norm) and its snapshot of the Adam state; workgroup 0 also
//                 copies the loss-scale state into the workspace, behind that snapshot.
//   k_adam_step_scaled   k_adam_step's work (adam_update) with e = grad_scale / S in f64, S from the snapshot, where it has
//                 grad_scale.  Lane 0 of workgroup 0 then writes the new loss-scale state from the snapshot.
// Race-free as hs_k_adam.h explains: the step reads snapshots, which only the norm launch writes, and writes the caller's
// states, which only the norm launch (and the next minibatch's loss kernels, ordered by the stream) read.  No scratch.
//
// Included ahead of hs_k_adam.h in hideseek.hip, as hs_k_gather.h and the others: every kernel here is a template, emitted
// where launch_adam_scaled (after the last of the other launch functions) names it.  The functions it calls are
// hs_k_adam.h's, hs_k_ppo.h's and hs_k_twohot.h's own, so those headers are included from here.
#pragma once
#include "hs_k_twohot.h"                  // twohot_samples, and through it hs_k_ppo.h: ppo_samples
#include "hs_k_adam.h"                    // adam_norm, adam_update

namespace hs {

constexpr int kLossScaleState = 4;                                      // S, good steps, backoffs, growths
constexpr int kLossScaleWorkspace = kAdamWorkspace + kLossScaleState;   // f64: hs_adam_step's workspace, then the snapshot of the loss-scale state
static_assert(kAdamThreads >= kLossScaleState, "a lane per state word");

struct LossScaleArgs {
    double *state;                        // [kLossScaleState]
    double growth, backoff, minScale, maxScale;
    double growthInterval;                // a whole number, compared with the count of good steps
};

template <typename TL, typename TG, typename TV>
__global__ __launch_bounds__(kPpoThreads) void k_ppo_scaled(PpoArgs a, const double *__restrict__ lossScale) {
    ppo_samples<TL, TG, TV>(a, [&] { return a.gradScale * (float)lossScale[0]; });
}

template <typename TL, typename TG, typename TV>
__global__ __launch_bounds__(kTwThreads) void k_twohot_scaled(TwohotArgs a, const double *__restrict__ lossScale) {
    twohot_samples<TL, TG, TV>(a, [&] { return a.gradScale * (float)lossScale[0]; });
}

template <int kThreads = kAdamThreads>
__global__ __launch_bounds__(kThreads) void k_adam_norm_scaled(const float *__restrict__ g, int n, const double *__restrict__ state,
                                                               const double *__restrict__ lossScale, double *__restrict__ ws) {
    adam_norm<kThreads>(g, n, ws, [=](int tid) {
        if (tid < kAdamState) ws[kAdamMaxGrid + tid] = state[tid];
        if (tid < kLossScaleState) ws[kAdamWorkspace + tid] = lossScale[tid];
    });
}

template <int kThreads = kAdamThreads>
__global__ __launch_bounds__(kThreads) void k_adam_step_scaled(AdamArgs a, LossScaleArgs ls) {
    const double *snap = a.ws + kAdamWorkspace;           // S, good steps, backoffs, growths as the norm launch found them
    adam_update<kThreads>(a, [&] { return a.gradScale / snap[0]; }, [&](bool skipped) {
        const double S = snap[0], good = snap[1], backoffs = snap[2], growths = snap[3];
        if (skipped) {
            const double down = S * ls.backoff;
            ls.state[0] = down > ls.minScale ? down : ls.minScale;
            ls.state[1] = 0.0;
            ls.state[2] = backoffs + 1.0;
        } else if (good + 1.0 >= ls.growthInterval) {
            const double up = S * ls.growth;
            ls.state[0] = up < ls.maxScale ? up : ls.maxScale;
            ls.state[1] = 0.0;
            ls.state[3] = growths + 1.0;
        } else {
            ls.state[1] = good + 1.0;
        }
    });
}

}  // namespace hs
