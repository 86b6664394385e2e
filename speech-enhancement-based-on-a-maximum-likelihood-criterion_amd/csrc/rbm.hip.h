// rbm.hip.h -- CD-1 pre-training of one hidden layer (rbm_rule.h): the session's own kernels, its launch sequence and
// the mlggd_rbm_* entries.  engine.hip includes it last: everything pre-training adds is read in one place, and an engine
// that never opens a session launches what it launched before and allocates nothing for it.
//
// One step is six kernels (l = 1) on the engine's stream:
//   k_transpose_in            v0 rows straight into the stacked visible factor Vs[0 .. B) and v0^T into Yt[0]
//                             (l > 1: the engine's forward launches of layers 1 .. l - 1, then one device copy of Y[l-1])
//   k_fwd<FWD_SIGMOID, 4, 4>  h0p = sigma(v0 W + b): the hidden forward's own kernel, unchanged
//   k_rbm_sample              h0s^T (the down-pass' operand) and -h0p into the stacked hidden factor Hs[0 .. B)
//   k_dx<4, P, ACT_VIS_*>     v1 = h0s W^T + c (or sigma of it): dx_body with the reconstruction epilogue; v1^T for the
//                             next up-pass and v1 rows into Vs[B .. 2 B).  P = 4 or 1: engine.hip dx_dma, as in run_dx
//   k_fwd<FWD_SIGMOID, 4, 4>  h1p = sigma(v1 W + b), rows into Hs[B .. 2 B)
//   k_rbm_vbias               dc, c and the step's float64 reconstruction partials (one per 32 visible units, fixed order)
//   k_dw<1, true>             g = Vs^T Hs at depth 2 B with dW, W, db and b updated in its epilogue: W and dW are read and
//                             written once per step
// Sampling is a launch of its own: the up-pass writes probabilities that the update needs unsampled, its epilogue is the
// training forward's and stays as it is, and the launch also forms -h0p where k_dw reads it, which would otherwise
// be a launch anyway.  The RBM's own three products always take the 32 x 32-tile kernels; MLGGD_TILE64 is honoured by the
// forward launches below layer l and ignored here.
#pragma once
#include <hip/hip_runtime.h>

#include "devbuf.h"
#include "kernels.hip.h"
#include "rbm_rule.h"

// h0p rows [Bp][Np] -> h0sT [Np][Bp] (zero pads) and neg rows [B][Np] = -h0p
__global__ __launch_bounds__(256) void k_rbm_sample(const float *__restrict__ h0p, float *__restrict__ h0sT,
                                                    float *__restrict__ neg, int B, int Bp, int N, int Np, unsigned seed,
                                                    unsigned step) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Bp * Np) return;
    const int b = (int)(idx / (unsigned)Np), j = (int)(idx % (unsigned)Np);
    const float p = h0p[idx];
    float s = 0.0f;
    if (b < B && j < N) s = rbm_rule::sample(rbm_rule::draw(seed, step, (unsigned)(b * N + j)), p);
    h0sT[(size_t)j * Bp + b] = s;
    if (b < B) neg[idx] = -p;
}

// The visible-bias update of rbm_rule.h and the reconstruction error over the stacked rows Vs = [v0; v1] (row stride Kp).
// A workgroup owns 32 visible units; its 8 strips of 32 threads each walk the frames b = strip, strip + 8, ... (a
// thread per unit and frame would be a 12-workgroup launch of B dependent loads: it took longer than the update GEMM),
// the strips' sums are added in strip order by the first strip, which also updates dc and c, and the 32 units' float64
// shares are added in unit order into partial[blockIdx.x]: a fixed order throughout, the same bits every run.
constexpr int RBM_VB_UNITS = 32, RBM_VB_STRIPS = 8;
__global__ __launch_bounds__(256) void k_rbm_vbias(const float *__restrict__ Vs, float *__restrict__ c, float *__restrict__ dc,
                                                   double *__restrict__ partial, int B, int K, int Kp, float nf, float mom,
                                                   float lr) {
    __shared__ float fs[RBM_VB_STRIPS][RBM_VB_UNITS];
    __shared__ double qs[RBM_VB_STRIPS][RBM_VB_UNITS];
    const int kl = (int)(threadIdx.x & 31), strip = (int)(threadIdx.x >> 5);
    const int k = (int)blockIdx.x * RBM_VB_UNITS + kl;
    float sum = 0.0f;
    double q = 0.0;
    if (k < K) {
#pragma unroll 4
        for (int b = strip; b < B; b += RBM_VB_STRIPS) {
            const float v0 = Vs[(size_t)b * Kp + k], v1 = Vs[(size_t)(B + b) * Kp + k];
            sum += rbm_rule::bias_term(v0, v1);
            q += rbm_rule::sqerr_term(v0, v1);
        }
    }
    fs[strip][kl] = sum;
    qs[strip][kl] = q;
    __syncthreads();
    if (strip == 0) {
        for (int s = 1; s < RBM_VB_STRIPS; s++) {
            sum += fs[s][kl];
            q += qs[s][kl];
        }
        if (k < K) {
            float d = dc[k], cv = c[k];
            rbm_rule::update_bias(sum, nf, mom, lr, &d, &cv);
            dc[k] = d;
            c[k] = cv;
        }
        qs[0][kl] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = qs[0][0];
        for (int u = 1; u < RBM_VB_UNITS; u++) tot += qs[0][u];
        partial[blockIdx.x] = tot;
    }
}

// out[0] = the n partials of a call added in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void k_rbm_fold(const double *__restrict__ partial, int n, double *__restrict__ out) {
    __shared__ double red[256];
    double q = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) q += partial[i];
    red[threadIdx.x] = q;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

struct mlggd_rbm {
    mlggd_engine *e = nullptr;
    int l = 0, visible = 0;
    float lr = 0, mom = 0, wc = 0;
    unsigned seed = 0, step = 0;
    int R = 0;  // rows of the stacked factors: ceil32(B + Bp), so that the pad frames of the second half have a place
    // H0 [Bp][Np] h0p rows; HT [Np][Bp] the up-passes' transposed output; H0sT [Np][Bp] samples; Hs [R][Np] = [-h0p; h1p];
    // Vs [R][Kp] = [v0; v1]; VT [Kp][Bp] v1^T; c, dc [Kp]; dW [Kp][Np], db [Np]: the session's momentum
    DevBuf<float> H0, HT, H0sT, Hs, Vs, VT, c, dc, dW, db;
    DevBuf<double> partial, total;
};

static int rbm_alloc(mlggd_rbm *r) {
    mlggd_engine *e = r->e;
    const size_t Kp = e->lsp[r->l - 1], Np = e->lsp[r->l], Bp = e->Bp, R = r->R;
    const hipStream_t *z = &e->stream;
    HIPCHK(r->H0.grow(Bp * Np, Bp * Np, e->bufs, z, nullptr));
    HIPCHK(r->HT.grow(Np * Bp, Np * Bp, e->bufs, z, nullptr));
    HIPCHK(r->H0sT.grow(Np * Bp, Np * Bp, e->bufs, z, nullptr));
    HIPCHK(r->Hs.grow(R * Np, R * Np, e->bufs, z, nullptr));
    HIPCHK(r->Vs.grow(R * Kp, R * Kp, e->bufs, z, nullptr));
    HIPCHK(r->VT.grow(Kp * Bp, Kp * Bp, e->bufs, z, nullptr));
    HIPCHK(r->c.grow(Kp, Kp, e->bufs, z, nullptr));
    HIPCHK(r->dc.grow(Kp, Kp, e->bufs, z, nullptr));
    HIPCHK(r->dW.grow(Kp * Np, Kp * Np, e->bufs, z, nullptr));
    HIPCHK(r->db.grow(Np, Np, e->bufs, z, nullptr));
    HIPCHK(r->total.grow(1, 1, e->bufs, z, nullptr));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}

static int rbm_vbias_blocks(const mlggd_rbm *r) { return (r->e->ls[r->l - 1] + RBM_VB_UNITS - 1) / RBM_VB_UNITS; }

// the hidden forward of layer l on the session's buffers: Yt_in [Kp][Bp] -> rows_out [Bp][Np] (and HT)
static int rbm_up(mlggd_rbm *r, const float *Yt_in, float *rows_out) {
    mlggd_engine *e = r->e;
    const int l = r->l;
    FwdArgs fa = fwd_args(e, l, rows_out);
    fa.Yt_in = Yt_in;
    fa.Yt_out = r->HT.p;
    fa.S = 1;
    fa.s_shift = 0;
    fa.yblk = 0;
    const dim3 grid(fa.n_tiles * fa.b_tiles);
    const size_t lds = fwd_lds_floats<4, 4>() * sizeof(float);
    CHK(ensure_lds(e, k_fwd<FWD_SIGMOID, 4, 4, false>, lds));
    hipLaunchKernelGGL((k_fwd<FWD_SIGMOID, 4, 4, false>), grid, dim3(256), lds, e->stream, fa, (long long *)nullptr);
    return launch_check("k_fwd (RBM up-pass)");
}

template <int ACT>
static int rbm_down_t(mlggd_rbm *r) {
    mlggd_engine *e = r->e;
    const int l = r->l, Kp = e->lsp[l - 1], b_tiles = e->Bp / 32;
    DxArgs xa = dx_args(e, l);
    xa.dEdXt = r->H0sT.p;
    xa.Yt_prev = r->c.p;  // the visible bias [Kp]
    xa.dEdXt_prev = r->VT.p;
    xa.dEdX_prev = r->Vs.p + (size_t)e->B * Kp;
    const dim3 grid((Kp / 32) * b_tiles);
    if (dx_dma(e, Kp)) {  // run_dx's choice between the two forms
        const size_t lds = dx_lds_floats<4, 4>() * sizeof(float);
        CHK(ensure_lds(e, k_dx<4, 4, ACT, false>, lds));
        hipLaunchKernelGGL((k_dx<4, 4, ACT, false>), grid, dim3(256), lds, e->stream, xa, (long long *)nullptr);
    } else {
        const size_t lds = dx_lds_floats<4, 1>() * sizeof(float);
        CHK(ensure_lds(e, k_dx<4, 1, ACT, false>, lds));
        hipLaunchKernelGGL((k_dx<4, 1, ACT, false>), grid, dim3(256), lds, e->stream, xa, (long long *)nullptr);
    }
    return launch_check("k_dx (RBM down-pass)");
}

// one CD-1 step on the bunch that starts at sample0 of the resident chunk; its partials go to slot `slot` of the call
static int rbm_step(mlggd_rbm *r, int sample0, int slot) {
    mlggd_engine *e = r->e;
    const int l = r->l, B = e->B, Bp = e->Bp;
    const int K = e->ls[l - 1], N = e->ls[l], Kp = e->lsp[l - 1], Np = e->lsp[l];
    const Bunch bn = bunch_at(e, sample0);
    if (l == 1) {
        hipLaunchKernelGGL(k_transpose_in, dim3(stage_blocks(e)), dim3(256), 0, e->stream, stage_args(e, bn, B, r->Vs.p));
        CHK(launch_check("k_transpose_in (RBM)"));
    } else {
        const int flag = e->cfg.dropoutflag;  // pre-training ignores the dropout flags
        e->cfg.dropoutflag = 0;
        const int rc = run_forward(e, bn, B, false, false, 0, l);
        e->cfg.dropoutflag = flag;
        CHK(rc);
        HIPCHK(hipMemcpyAsync(r->Vs.p, e->Y[l - 1], (size_t)B * Kp * 4, hipMemcpyDeviceToDevice, e->stream));
    }
    CHK(rbm_up(r, e->Yt[l - 1], r->H0.p));
    {
        const size_t n = (size_t)Bp * Np;
        hipLaunchKernelGGL(k_rbm_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, (const float *)r->H0.p,
                           r->H0sT.p, r->Hs.p, B, Bp, N, Np, r->seed, r->step);
        CHK(launch_check("k_rbm_sample"));
    }
    CHK(r->visible == rbm_rule::kGaussian ? rbm_down_t<ACT_VIS_LINEAR>(r) : rbm_down_t<ACT_VIS_SIGMOID>(r));
    CHK(rbm_up(r, r->VT.p, r->Hs.p + (size_t)B * Np));
    const int B2 = 2 * B, B2p = ceil32(B2);
    if (B2p > B2)  // the second up-pass' pad frames landed in the rows k_dw still reads: exact zeros there
        HIPCHK(hipMemsetAsync(r->Hs.p + (size_t)B2 * Np, 0, (size_t)(B2p - B2) * Np * 4, e->stream));
    const int vb = rbm_vbias_blocks(r);
    hipLaunchKernelGGL(k_rbm_vbias, dim3(vb), dim3(256), 0, e->stream, (const float *)r->Vs.p, r->c.p, r->dc.p,
                       r->partial.p + (size_t)slot * vb, B, K, Kp, (float)B, r->mom, r->lr);
    CHK(launch_check("k_rbm_vbias"));
    {
        const int n_wg = (Np + 63) / 64, k_wg = (Kp + 63) / 64;
        const size_t lds = (size_t)2 * 64 * 64 * sizeof(float);
        CHK(ensure_lds(e, k_dw<1, true>, lds));
        hipLaunchKernelGGL((k_dw<1, true>), dim3(k_wg * n_wg), dim3(256), lds, e->stream, (const float *)r->Vs.p, Kp,
                           (const float *)r->Hs.p, e->W[l], r->dW.p, (float *)nullptr, e->bias[l], r->db.p, (float *)nullptr,
                           K, N, Np, B2, B2p, n_wg, (float)B, r->mom, r->lr, r->wc, (long long *)nullptr);
        CHK(launch_check("k_dw (RBM update)"));
    }
    r->step++;
    return MLGGD_OK;
}

// every full bunch of the resident chunk of n samples
static int rbm_train_resident(mlggd_rbm *r, int n, int *bunches, double *recon_sqerr) {
    mlggd_engine *e = r->e;
    const int steps = n / e->B, vb = rbm_vbias_blocks(r);
    double tot = 0.0;
    if (steps > 0) {
        const size_t need = (size_t)steps * vb;
        HIPCHK(r->partial.grow(need, need, e->bufs, nullptr, &e->stream));
        HIPCHK(hipEventRecord(e->ev_t0, e->stream));  // mlggd_last_train_ms then times this call's steps
        for (int s = 0; s < steps; s++) CHK(rbm_step(r, s * e->B, s));
        hipLaunchKernelGGL(k_rbm_fold, dim3(1), dim3(256), 0, e->stream, (const double *)r->partial.p, steps * vb, r->total.p);
        CHK(launch_check("k_rbm_fold"));
        HIPCHK(hipEventRecord(e->ev_t1, e->stream));
        e->last_steps = steps;
        e->timing_valid = true;
        HIPCHK(hipMemcpyAsync(&tot, r->total.p, sizeof(double), hipMemcpyDeviceToHost, e->stream));
        if (e->indexed && e->copy_stream) HIPCHK(hipEventRecord(e->raw[e->raw_cur].last_use, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    if (bunches) *bunches = steps;
    if (recon_sqerr) *recon_sqerr = tot;
    return MLGGD_OK;
}

extern "C" {

int mlggd_rbm_open(mlggd_handle e, int layer, int visible, float lrate, float momentum, float weightcost, uint32_t seed,
                   mlggd_rbm_handle *out) {
    if (!e || !out) return fail(MLGGD_ERR_ARG, "NULL handle / out");
    *out = nullptr;
    if (!rbm_rule::valid_layer(layer, e->L))
        return fail(MLGGD_ERR_ARG, "mlggd_rbm_open: layer %d is not a hidden layer 1..%d (the output layer is never pre-trained)",
                    layer, e->L - 2);
    if (!rbm_rule::valid_visible(visible))
        return fail(MLGGD_ERR_ARG, "mlggd_rbm_open: visible %d is neither MLGGD_RBM_GAUSSIAN nor MLGGD_RBM_BERNOULLI", visible);
    if (e->cfg.activation != MLGGD_ACT_SIGMOID)
        return fail(MLGGD_ERR_STATE, "mlggd_rbm_open: pre-training of a rectified-linear engine is not built");
    if (e->nat_frames > 0)
        return fail(MLGGD_ERR_STATE, "mlggd_rbm_open: pre-training of an engine with nat_frames = %d is not built", e->nat_frames);
    CHK(check_single_device(e, "mlggd_rbm_open", true));
    if (e->rbm_open > 0) return fail(MLGGD_ERR_STATE, "mlggd_rbm_open: this engine already has an open RBM session");
    HIPCHK(hipSetDevice(e->device));
    mlggd_rbm *r = new mlggd_rbm;
    r->e = e, r->l = layer, r->visible = visible, r->lr = lrate, r->mom = momentum, r->wc = weightcost, r->seed = seed;
    r->R = ceil32(e->B + e->Bp);
    const int rc = rbm_alloc(r);
    if (rc != MLGGD_OK) {
        hipStreamSynchronize(e->stream);
        delete r;
        return rc;
    }
    e->rbm_open++;
    *out = r;
    return MLGGD_OK;
}

int mlggd_rbm_set_rates(mlggd_rbm_handle r, float lrate, float momentum) {
    if (!r) return fail(MLGGD_ERR_ARG, "NULL handle");
    r->lr = lrate, r->mom = momentum;
    return MLGGD_OK;
}

int mlggd_rbm_train_chunk(mlggd_rbm_handle r, int n_frames, const float *in, int *bunches, double *recon_sqerr) {
    if (!r) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (n_frames > 0 && !in) return fail(MLGGD_ERR_ARG, "in is NULL");
    CHK(mlggd_load_chunk(r->e, n_frames, in, nullptr));
    return rbm_train_resident(r, n_frames, bunches, recon_sqerr);
}

int mlggd_rbm_train_frames(mlggd_rbm_handle r, int n_frames, int fea_context, const float *feat, int n_samples,
                           const int32_t *first_frame, int *bunches, double *recon_sqerr) {
    if (!r) return fail(MLGGD_ERR_ARG, "NULL handle");
    CHK(mlggd_load_frames(r->e, n_frames, fea_context, feat, nullptr, n_samples, first_frame, 0));
    return rbm_train_resident(r, n_samples, bunches, recon_sqerr);
}

int mlggd_rbm_visible_bias(mlggd_rbm_handle r, float *c) { return mlggd_rbm_debug_tensor(r, "vbias", c, r ? (size_t)r->e->ls[r->l - 1] : 0); }

int mlggd_rbm_debug_tensor(mlggd_rbm_handle r, const char *name, float *dst, size_t count) {
    if (!r || !name || !dst) return fail(MLGGD_ERR_ARG, "NULL argument");
    mlggd_engine *e = r->e;
    HIPCHK(hipSetDevice(e->device));
    const int l = r->l, B = e->B, Bp = e->Bp, K = e->ls[l - 1], N = e->ls[l], Kp = e->lsp[l - 1], Np = e->lsp[l];
    const std::string nm(name);
    auto need = [&](size_t n) -> int {
        return count < n ? fail(MLGGD_ERR_ARG, "dst holds %zu floats, %s needs %zu", count, name, n) : MLGGD_OK;
    };
    // rows [B][U] out of a row-major device matrix of row stride Up
    auto rows = [&](const float *src, int U, int Up) -> int {
        CHK(need((size_t)B * U));
        HIPCHK(hipMemcpy2DAsync(dst, (size_t)U * 4, src, (size_t)Up * 4, (size_t)U * 4, B, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return MLGGD_OK;
    };
    auto vec = [&](const float *src, int U) -> int {
        CHK(need((size_t)U));
        HIPCHK(hipMemcpyAsync(dst, src, (size_t)U * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return MLGGD_OK;
    };
    if (nm == "v0") return rows(r->Vs.p, K, Kp);
    if (nm == "v1") return rows(r->Vs.p + (size_t)B * Kp, K, Kp);
    if (nm == "h0p") return rows(r->H0.p, N, Np);
    if (nm == "h1p") return rows(r->Hs.p + (size_t)B * Np, N, Np);
    if (nm == "h0s") {  // kept transposed [Np][Bp]
        CHK(need((size_t)B * N));
        std::vector<float> t((size_t)Np * Bp);
        HIPCHK(hipMemcpyAsync(t.data(), r->H0sT.p, t.size() * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (int b = 0; b < B; b++)
            for (int n = 0; n < N; n++) dst[(size_t)b * N + n] = t[(size_t)n * Bp + b];
        return MLGGD_OK;
    }
    if (nm == "delta_w") {
        CHK(need((size_t)K * N));
        CHK(download_padded(dst, r->dW.p, Np, K, N, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return MLGGD_OK;
    }
    if (nm == "delta_b") return vec(r->db.p, N);
    if (nm == "delta_c") return vec(r->dc.p, K);
    if (nm == "vbias") return vec(r->c.p, K);
    return fail(MLGGD_ERR_ARG, "unknown RBM tensor name '%s'", name);
}

int mlggd_rbm_draws(uint32_t seed, uint32_t step, int B, int N, float *out) {
    if (B < 0 || N < 0 || (long long)B * N > INT32_MAX) return fail(MLGGD_ERR_ARG, "mlggd_rbm_draws: B %d x N %d", B, N);
    if ((long long)B * N > 0 && !out) return fail(MLGGD_ERR_ARG, "r is NULL");
    rbm_rule::draws(seed, step, B, N, out);
    return MLGGD_OK;
}

int mlggd_rbm_close(mlggd_rbm_handle r) {
    if (!r) return MLGGD_OK;
    mlggd_engine *e = r->e;
    hipSetDevice(e->device);
    hipStreamSynchronize(e->stream);
    e->rbm_open--;
    delete r;  // every DevBuf gives its bytes back
    return MLGGD_OK;
}

}  // extern "C"
