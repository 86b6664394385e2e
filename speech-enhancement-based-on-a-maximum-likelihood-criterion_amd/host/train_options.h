// train_options.h -- everything the trainer (bptrain_main.cc) reads from its environment, read once and checked before a
// device is opened or a chunk is trained: a bad value, a bad file or a run the option does not fit ends the run with
// one message.  None of it is in the reference: the 28-key command line, the log file and the weights' format do not
// change, and a run without a variable is the run it was.  An empty value counts as unset (MLGGD_TIMING apart).
//
// The reader depends on the parsed command line and on a few small files only, and calls nothing of libmlggd.so, so
// tests/host_api.cc runs it over a table of NAME=VALUE strings without a GPU (tests/test_trainer_options.py).
#pragma once
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "../csrc/adam_rule.h"
#include "../csrc/scale_rule.h"
#include "optfile.h"
#include "trainer_io.h"

namespace mlggd_host {

// name -> value or nullptr: the process environment in the program, a table in the tests
using EnvLookup = std::function<const char *(const char *)>;

// What main() needs before it parses its command line (only rank 0 opens the log and the weights file).
struct LaunchEnv {
    // Data parallel: torchrun-style WORLD_SIZE, RANK and LOCAL_RANK, the last defaulting to the rank.
    // With world > 1 every rank reads the same chunks with the same seed and trains rows
    // [rank*bunchsize,(rank+1)*bunchsize) of each global minibatch of world*bunchsize samples; rank 0 alone writes the
    // log, the weights and runs CV; local_rank names the device.
    int world = 1, rank = 0, local_rank = 0;
    // MLGGD_TIMING (set, to whatever value -- the one variable whose empty value counts): wall-clock of the phases on stderr
    bool timing = false;
};
LaunchEnv read_launch_env(const EnvLookup &env = getenv);

struct TrainOptions : LaunchEnv {
    // Input pipeline: by default chunks travel as raw normalised frames plus the first frame of every
    // (shuffled) sample row and are gathered on the GPU; MLGGD_EXPANDED=1 (frames = false) selects the reference's
    // host-side context expansion (Interface::Readchunk) instead -- same results.  MLGGD_PINNED=0: the frame buffers
    // are not page-locked.
    bool frames = true, pinned = true;
    // MLGGD_WATCHDOG_S (0: off): seconds without progress after which a data-parallel rank gives up (bptrain_main.cc)
    int watchdog_s = 900;
    // MLGGD_ID_FILE names a file on a shared filesystem used to hand the RCCL unique id from rank 0 to the others
    // (dp_launch.h); MLGGD_RENDEZVOUS_TIMEOUT: seconds a rank waits there
    std::string id_file;
    int rendezvous_timeout = 600;

    // Error model (errmodel.h): with MLGGD_ERRMODEL=FILE rank 0 makes a second pass over the CV chunks after the three CV
    // log lines, adds their error statistics (mlggd_error_stats: per-bin sums of e^1..4 and |e|^beta over the grid of
    // MLGGD_ERRMODEL_BETAS=lo:step:hi, default 0.5:0.1:2.5), fits the GGD per bin and shared (mlggd_ggd_fit) and writes
    // FILE; one stdout line names the file and the shared beta -- the value for `shapefactor`.
    std::string errmodel_fn;
    // Asymmetric error model (asymfile.h): with MLGGD_ASYMMODEL=FILE rank 0 makes one more pass over the CV chunks after
    // the epoch (mlggd_error_stats_signed over the same grid, added, mlggd_asym_fit) and writes a shape and a skew per bin
    // to FILE; the file reads as a shape file too.  One fit feeds MLGGD_SHAPEFACTORS=fit.txt MLGGD_ASYMMETRY=fit.txt in
    // the next epoch.
    std::string asymmodel_fn;
    // the grid of both models, parsed on rank 0 when either is asked for: a bad grid ends the run before the epoch, not
    // after it; empty on every other rank, which never looks at the variable
    std::vector<float> model_betas;
    // Global variance (gvfile.h): with MLGGD_GVFILE=FILE rank 0 makes one more pass over the CV chunks after the error
    // models' (all may be set in one run), adds their output statistics (mlggd_output_stats: per-bin sums of y, y^2, t,
    // t^2 of the normalised outputs and targets), fits the equalisation factors per bin and shared (mlggd_gv_fit) and
    // writes FILE for the decoders' gv=FILE; one stdout line names the file and the shared factor.
    std::string gv_fn;

    // Per-bin shapes: with MLGGD_SHAPEFACTORS=FILE every rank reads one shape per output bin from FILE -- a plain list
    // of D numbers or the file MLGGD_ERRMODEL wrote in an earlier epoch (its best_beta column; a bin without a fit takes
    // the file's shared beta, else `shapefactor`) -- and sets it on the engine before the first chunk
    // (mlggd_set_shapefactors).  One stderr line names the file and the minimum, maximum and mean shape; the form of the
    // log lines does not change, the CV log likelihood is then the vector's.  Needs MLflag=1.
    std::string shapes_fn;
    std::vector<float> shapes;  // [D], empty without the variable
    // Skews: with MLGGD_ASYMMETRY=FILE every rank reads one skew per output bin from FILE -- a plain list of D numbers or
    // the file MLGGD_ASYMMODEL wrote (its best_kappa column; a bin without a fit takes 1) -- and sets it on the engine
    // before the first chunk (mlggd_set_asymmetry); one stderr line names the file and the minimum, maximum and mean
    // skew.  Needs MLflag=1.
    std::string asym_fn;
    std::vector<float> skews;  // [D], empty without the variable

    // Learned scale (scalefile.h, csrc/scale_rule.h): with MLGGD_SCALE=learned (`alternating`: the default by name) every
    // rank switches the engine to the learned scale before the first chunk (mlggd_set_scale_mode; MLGGD_SCALE_LRATE,
    // MLGGD_SCALE_MOMENTUM and MLGGD_SCALE_VMAX are optional).  finetune.pl starts one process per epoch and a .wts file
    // has no place for alpha, so the state travels in a file: MLGGD_SCALE_FILE=PATH is read before the first chunk if it
    // exists -- without it the first epoch seeds every bin from its first minibatch -- and written by rank 0 after the
    // epoch's CV pass.  One stderr line names the rates and the state's origin, one stdout line the file written.
    // Needs MLflag=1.
    bool scale_learned = false;
    std::string scale_fn;
    float scale_lrate = scale_rule::kLrate, scale_momentum = scale_rule::kMomentum, scale_vmax = scale_rule::kVmax;
    std::vector<float> scale_alpha, scale_velocity;  // [D] each: the state the file held, empty: none
    long long scale_steps0 = 0;                       // the steps that state has behind it

    // Adam (optfile.h, csrc/adam_rule.h): with MLGGD_OPTIMIZER=adam (`sgd`: the default by name) the engine is switched to
    // Adam before the first chunk (mlggd_set_optimizer; MLGGD_ADAM_BETA1, MLGGD_ADAM_BETA2 and MLGGD_ADAM_EPS are
    // optional); lrate is then the Adam rate and momentum is ignored.  An optimizer with a state is useless across
    // one-process-per-epoch runs unless the state travels too: MLGGD_OPT_FILE=PATH (binary) is read before the first
    // chunk if it exists -- without it the moments start from zero, a file for another net ends the run -- and written
    // after the epoch's weights file.  One stderr line names the parameters and the state's origin, one stdout line the
    // file written.  A single rank only: WORLD_SIZE > 1 is refused naming the variable.
    bool adam = false;
    std::string opt_fn;
    float adam_beta1 = adam_rule::kBeta1, adam_beta2 = adam_rule::kBeta2, adam_eps = adam_rule::kEps;
    OptState opt_state;  // what the file held: its own betas and eps describe the run that wrote it
    bool opt_restored = false;
};

// Throws where a check fails, and only the first fault is reported, in this order: the error model's grid; the shapes
// (MLflag, then the file); the asymmetric model's grid; the skews likewise; the scale (mode word, file without the
// mode, MLflag, a rate that is no number, the rates' ranges, the state file); the optimizer (kind, file without Adam,
// several ranks, a parameter that is no number, the parameters' ranges, the state file).
TrainOptions read_train_options(const WorkPara &p, int numlayers, const EnvLookup &env = getenv);

}  // namespace mlggd_host
