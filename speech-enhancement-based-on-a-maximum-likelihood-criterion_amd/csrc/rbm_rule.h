// rbm_rule.h -- layer-wise pre-training of a sigmoid net by one-step contrastive divergence (Hinton; the initialisation of
// Xu, Du, Dai and Lee's regression DNN: a Gaussian-Bernoulli RBM on the z-normalised input, Bernoulli-Bernoulli RBMs
// above it), stated once for host and device (rbm.hip.h, mlggd_rbm_*).  Plain C++ with no device call, so that it also
// builds into a stand-alone host program.  All values are fp32 unless said otherwise, every statement is one IEEE
// operation, nothing is contracted (-ffp-contract=off).
//
// An RBM is opened on hidden layer l of an engine, 1 <= l <= numlayers - 2 (the output layer is never pre-trained).
// W [K][N] is the engine's weight matrix into layer l, b [N] that layer's bias, c [K] a visible bias the session owns
// (0 at open), B the engine's bunchsize.  One step on a minibatch, `step` counting the session's steps from 0:
//   v0  [B][K]  l = 1: the staged input rows; l > 1: the activations of layer l - 1 from the engine's ordinary
//               deterministic forward pass through layers 1 .. l - 1 (probabilities, never samples; no dropout)
//   h0p [B][N]  sigma(v0 W + b): the hidden forward of layer l, sigmoid_det included
//   h0s [B][N]  (r < h0p) ? 1 : 0 with r = draw(seed, step, b * N + j): the index knows no padding
//   v1  [B][K]  gaussian (unit variance): h0s W^T + c;  bernoulli: sigma(h0s W^T + c).  Never sampled.
//   h1p [B][N]  sigma(v1 W + b)
//   g   [K][N]  sum_b (v1^T h1p - v0^T h0p): the statistics use h0p, not h0s; one 2 B deep product [v0; v1]^T [-h0p; h1p]
//   dW = mom * dW - lr * (g / B + wc * W);  W = dW + 1.0f * W                  k_apply_update's form
//   db = mom * db - lr * (sum_b (h1p - h0p) / B);  b = db + 1.0f * b           summed over the rows of [-h0p; h1p] in order
//   dc = mom * dc - lr * (sum_b (v1 - v0) / B);    c = dc + c                  update_bias(): a fixed order of the frames
// Bias terms carry no weight cost, as in training.  dW, db and dc are the session's own momentum state (0 at open); the
// engine's fine-tuning momentum is not touched.  The reconstruction error of a step is sum_b sum_k (v0 - v1)^2 with the
// difference, its square and the sum in float64 and a fixed order, so that the same input gives the same bits.  A
// trailing partial bunch is skipped.  Not built, and refused: CD-k for k > 1, persistent chains, sampled visibles,
// learnt variances, rectified-linear, noise-aware and multi-device engines.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RBM_HD __host__ __device__
#else
#define RBM_HD
#endif

namespace rbm_rule {

constexpr int kGaussian = 0, kBernoulli = 1;  // MLGGD_RBM_GAUSSIAN / MLGGD_RBM_BERNOULLI

// the generator of k_dropout (kernels.hip.h), restated: a counter-based hash
RBM_HD inline uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// r in [0, 1): 24 bits, exact in fp32
RBM_HD inline float draw(uint32_t seed, uint32_t step, uint32_t idx) {
    const uint32_t hsh = mix32(mix32(seed ^ (step * 0x9e3779b9u)) ^ idx);
    return (float)(hsh >> 8) * (1.0f / 16777216.0f);
}

// h0s from its draw and h0p; a NaN probability gives 0
RBM_HD inline float sample(float r, float p) { return r < p ? 1.0f : 0.0f; }

// one more frame into a visible unit's sum_b (v1 - v0)
RBM_HD inline float bias_term(float v0, float v1) { return v1 - v0; }

// dc, then c, from the unit's sum over the B frames; nf = (float)B
RBM_HD inline void update_bias(float sum, float nf, float mom, float lr, float *dc, float *c) {
    const float mean = sum / nf;
    const float keep = mom * *dc;
    const float step = lr * mean;
    const float d = keep - step;
    *dc = d;
    *c = d + *c;
}

// one element's share of the reconstruction error
RBM_HD inline double sqerr_term(float v0, float v1) {
    const double d = (double)v0 - (double)v1;
    return d * d;
}

// what mlggd_rbm_open accepts of (layer, visible) on a net of L layers
inline bool valid_layer(int layer, int L) { return layer >= 1 && layer <= L - 2; }
inline bool valid_visible(int visible) { return visible == kGaussian || visible == kBernoulli; }

// r [B][N] of one step on the host
inline void draws(uint32_t seed, uint32_t step, int B, int N, float *r) {
    for (size_t i = 0; i < (size_t)B * (size_t)N; i++) r[i] = draw(seed, step, (uint32_t)i);
}

}  // namespace rbm_rule
