// bp_gpu.h -- a `class BP_GPU` with the reference's constructor and public methods
// (Train_code_ML_GGD/BP_GPU.h:45-70) implemented as a thin C++ shim over the C-ABI of
// include/mlggd.h, so a main() written against the reference class compiles against the
// MI355X engine unchanged.  Error behaviour: the reference printf()s and exit(0)s
// (BP_GPU.cu:20,534,578); the shim prints the engine's message and exit(1)s.
#pragma once
#include "../../include/mlggd.h"

class BP_GPU {
  public:
    BP_GPU(int random_seed, int a_GPU_selected, int a_numlayers, int *a_layersizes, int a_bunchsize, float a_lrate,
           float a_momentum, float a_weightcost, float **weights, float **bias, float shapefactor, int MLflag,
           int dropoutflag, float visible_omit, float hid_omit, int activation = MLGGD_ACT_SIGMOID);
    ~BP_GPU();
    void train(int n_frames, float *in, const float *targ);
    // One SGD step on n_frames = bunchsize rows (BP_GPU.h:53, BP_GPU.cu:308-440).  The reference's member is public
    // but takes pointers into its private device workspace (train passes dev.in + offset, BP_GPU.cu:170-184), so no
    // outside caller can use it there; here it takes HOST rows like train() does: upload + one step + wait.
    void train_bunch_single(int n_frames, float *in, const float *targ);
    float CrossValid(int n_frames, const float *in, const float *targ);
    float CrossValiddB(int n_frames, const float *in, const float *targ);
    float CrossValid2(int n_frames, const float *in, const float *targ);
    // one forward pass for all three metrics (same accumulation order as the three above)
    void CrossValidAll(int n_frames, const float *in, const float *targ, float *sqerr, float *abserr, float *loglik);
    void cv_bunch_single(int n_frames, const float *in, float *out);
    // frame-stream chunks (not in the reference): rows gathered on the device, see mlggd_load_frames
    // wait = false: return once the chunk is uploaded (the buffers are free) and its steps are enqueued; the next
    // chunk's upload then overlaps them.  sync() / returnWeights / CrossValid* wait for everything.
    void train_frames(int n_frames, int fea_context, const float *feat, const float *targ, int n_samples,
                      const int *first_frame, int targ_offset, bool wait = true);
    void sync();
    void CrossValidAll_frames(int n_frames, int fea_context, const float *feat, const float *targ, int n_samples,
                              const int *first_frame, int targ_offset, float *sqerr, float *abserr, float *loglik);
    // error statistics of a CV chunk (not in the reference): sums [4 + n_betas][D] of e^1..4 and |e|^beta per output
    // bin, overwritten; see mlggd_error_stats.  Needs a single-device engine without dropout.
    void ErrorStats(int n_frames, const float *in, const float *targ, int n_betas, const float *betas, double *sums);
    void ErrorStats_frames(int n_frames, int fea_context, const float *feat, const float *targ, int n_samples,
                           const int *first_frame, int targ_offset, int n_betas, const float *betas, double *sums);
    // output statistics of a CV chunk (not in the reference): sums [4][D] of y, y^2, t, t^2 per output bin, overwritten;
    // see mlggd_output_stats.  Needs a single-device engine without dropout.
    void OutputStats(int n_frames, const float *in, const float *targ, double *sums);
    void OutputStats_frames(int n_frames, int fea_context, const float *feat, const float *targ, int n_samples,
                            const int *first_frame, int targ_offset, double *sums);
    // one shape per output bin from the next step or CV call on (not in the reference; MLflag 1 only), nullptr: back
    // to `shapefactor`; see mlggd_set_shapefactors
    void setShapefactors(const float *betas);
    // the asymmetric error model (not in the reference; MLflag 1 only): one skew per output bin from the next step or
    // CV call on, nullptr: off (mlggd_set_asymmetry); its sufficient statistics [2 n_betas][D] of a CV chunk
    void setAsymmetry(const float *kappas);
    void ErrorStatsSigned(int n_frames, const float *in, const float *targ, int n_betas, const float *betas, double *sums);
    void ErrorStatsSigned_frames(int n_frames, int fea_context, const float *feat, const float *targ, int n_samples,
                                 const int *first_frame, int targ_offset, int n_betas, const float *betas, double *sums);
    // the learned scale (not in the reference; MLflag 1 only): alpha per output bin as a state moved by SGD beside the
    // weights (mlggd_set_scale_mode with MLGGD_SCALE_LEARNED), its state [D] + [D] and the steps it has taken
    void setScaleLearned(float lrate, float momentum, float vmax);
    void getScaleState(float *alpha, float *velocity);
    void setScaleState(const float *alpha, const float *velocity);
    long long scaleSteps();
    // (new, opt-in; not in the reference) Adam beside SGD with momentum (mlggd_set_optimizer with MLGGD_OPT_ADAM): the
    // moments in returnWeights' shapes and pointer arrays (slot 0 unused), and the updates taken
    void setOptimizerAdam(float beta1, float beta2, float eps);
    void getOptimizerState(float **m_w, float **v_w, float **m_b, float **v_b);
    void setOptimizerState(float **m_w, float **v_w, float **m_b, float **v_b, long long steps);
    long long optimizerSteps();
    void returnWeights(float **weights, float **bias);
    float Gamma(float x) { return mlggd_gamma(x); }
    // data parallel (not in the reference): join an RCCL communicator of `world` ranks
    void joinComm(const void *unique_id, int world, int rank);
    mlggd_handle handle() { return h_; }

    int numlayers;
    int layersizes[MLGGD_MAXLAYER];
    int bunchsize;
    float lrate, shapefactor, momentum, weightcost;
    int dropoutflag, MLflag;
    float visible_omit, hid_omit;
    int activation;  // MLGGD_ACT_SIGMOID (the reference's class) or MLGGD_ACT_RELU: not in the reference

  private:
    void check(int rc, const char *what);
    mlggd_handle h_ = nullptr;
};
