// bptrain_main.cc -- the trainer executable (drop-in for the reference's BPtrain_Sigmoid,
// Train_code_ML_GGD/BPtrain.cc:55-146): same key=value command line as emitted by
// finetune.pl:50-76, same log lines, same .wts output; one epoch per process.
//
// Flow (BPtrain.cc:74-145): Initial -> BP_GPU -> get_pfile_info -> plan training chunks ->
// shuffle the chunk order (one lrand48 stream: chunk order first, then one shuffle per chunk
// read, in read order) -> prefetch thread reads chunk i+1 while the GPU trains on chunk i ->
// write weights -> cross-validate -> three log lines.
//
// Input pipeline (new): by default chunks travel as raw normalised frames plus the
// first frame of every (shuffled) sample row and are gathered on the GPU; MLGGD_EXPANDED=1 selects
// the reference's host-side context expansion (Interface::Readchunk) instead -- same results.
//
// Error model (new, opt-in): with MLGGD_ERRMODEL=FILE rank 0 makes a second pass over the CV chunks after the three CV
// log lines, adds their error statistics (mlggd_error_stats: per-bin sums of e^1..4 and |e|^beta over the grid of
// MLGGD_ERRMODEL_BETAS=lo:step:hi, default 0.5:0.1:2.5), fits the GGD per bin and shared (mlggd_ggd_fit) and writes
// FILE (errmodel.h); one stdout line names the file and the shared beta -- the value for `shapefactor`.  The
// command line, the log file and the weights do not change.
//
// Global variance (new, opt-in): with MLGGD_GVFILE=FILE rank 0 makes one more pass over the CV chunks after the error
// model's (both may be set in one run), adds their output statistics (mlggd_output_stats: per-bin sums of y, y^2, t,
// t^2 of the normalised outputs and targets), fits the equalisation factors per bin and shared (mlggd_gv_fit) and
// writes FILE (gvfile.h) for the decoders' gv=FILE; one stdout line names the file and the shared factor.  The command
// line, the log file and the weights do not change.
//
// Per-bin shapes (new, opt-in): with MLGGD_SHAPEFACTORS=FILE every rank reads one shape per output bin from FILE -- a
// plain list of D numbers or the file MLGGD_ERRMODEL wrote in an earlier epoch (its best_beta column; a bin without a
// fit takes the file's shared beta, else `shapefactor`) -- and sets it on the engine before the first chunk
// (mlggd_set_shapefactors).  One stderr line names the file and the minimum, maximum and mean shape; the command line
// and the form of the log lines do not change, the CV log likelihood is then the vector's.  Needs MLflag=1.
//
// Activation (new): activation=sigmoid|relu selects the hidden units (mlggd_config.activation).  Without the key the
// program's own name decides: installed as BPtrain_ReLU -- the same program -- it trains rectified-linear nets, under
// any other name sigmoid ones, so a finetune.pl edited only in its $exe line trains a ReLU net.  Any other value ends
// the run before a file or a device is opened.  The banner line names the choice; the log file does not change.
//
// Asymmetric error model (new, opt-in; asymfile.h): with MLGGD_ASYMMODEL=FILE rank 0 makes one more pass over the CV
// chunks after the epoch (mlggd_error_stats_signed over the grid of MLGGD_ERRMODEL_BETAS, added, mlggd_asym_fit) and
// writes a shape and a skew per bin to FILE; the file reads as a shape file too.  With MLGGD_ASYMMETRY=FILE every
// rank reads one skew per output bin from FILE -- a plain list of D numbers or that file (its best_kappa column; a bin
// without a fit takes 1) -- and sets it on the engine before the first chunk (mlggd_set_asymmetry); one stderr line
// names the file and the minimum, maximum and mean skew.  Needs MLflag=1.  One fit feeds
// MLGGD_SHAPEFACTORS=fit.txt MLGGD_ASYMMETRY=fit.txt in the next epoch.
//
// Learned scale (new, opt-in; scalefile.h, csrc/scale_rule.h): with MLGGD_SCALE=learned every rank switches the engine
// to the learned scale before the first chunk (mlggd_set_scale_mode; MLGGD_SCALE_LRATE, MLGGD_SCALE_MOMENTUM and
// MLGGD_SCALE_VMAX are optional).  finetune.pl starts one process per epoch and a .wts file has no place for alpha, so
// the state travels in a file: MLGGD_SCALE_FILE=PATH is read before the first chunk if it exists, and written by rank 0
// after the epoch's CV pass.  One stderr line names the rates and the state's origin, one stdout line the file written.
// Needs MLflag=1; the log file and the weights' format do not change.
//
// Adam (new, opt-in; optfile.h, csrc/adam_rule.h): with MLGGD_OPTIMIZER=adam the engine is switched to Adam before the
// first chunk (mlggd_set_optimizer; MLGGD_ADAM_BETA1, MLGGD_ADAM_BETA2 and MLGGD_ADAM_EPS are optional); lrate is then the
// Adam rate and momentum is ignored.  An optimizer with a state is useless across one-process-per-epoch runs unless the
// state travels too: MLGGD_OPT_FILE=PATH (binary, optfile.h) is read before the first chunk if it exists -- a file for
// another net ends the run -- and written after the epoch's weights file.  One stderr line names the parameters and the
// state's origin, one stdout line the file written.  A single rank only: WORLD_SIZE > 1 is refused naming the variable.
// The log file and the weights' format do not change.
//
// Data parallel (new): when WORLD_SIZE > 1 (torchrun-style env: RANK,
// LOCAL_RANK, WORLD_SIZE; MLGGD_ID_FILE names a file on a shared filesystem used to hand the
// RCCL unique id from rank 0 to the others) every rank reads the same chunks with the same
// seed and trains rows [rank*bunchsize,(rank+1)*bunchsize) of each global minibatch of
// WORLD_SIZE*bunchsize samples; rank 0 alone writes the log, the weights and runs CV.
#include <chrono>
#include <condition_variable>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <unistd.h>

#include "bp_gpu.h"
#include "dp_launch.h"
#include "errmodel.h"
#include "asymfile.h"
#include "gvfile.h"
#include "scalefile.h"
#include "../csrc/scale_rule.h"
#include "optfile.h"
#include "../csrc/adam_rule.h"
#include "prefetch.h"
#include "trainer_io.h"

using mlggd_host::Interface;
using mlggd_host::IoError;
using mlggd_host::WorkPara;

namespace {

using mlggd_host::Slot;

std::atomic<bool> g_stop_fetch{false};  // set when the trainer gives up before consuming every chunk
int g_pinned_device = 0;                // device whose context owns the page-locked chunk buffers
std::string g_pinned_error;             // engine's message when a page-locked allocation failed (fetch thread only)

int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

// rank 0 creates the RCCL id and hands it to the other ranks through MLGGD_ID_FILE (dp_launch.h: a handshake
// with per-launch nonces, so a file left by an earlier epoch's launch is never accepted)
void exchange_id(int world, int rank, unsigned char id[MLGGD_UNIQUE_ID_BYTES]) {
    static_assert(MLGGD_UNIQUE_ID_BYTES == mlggd_host::kUniqueIdBytes, "id size");
    const char *path = getenv("MLGGD_ID_FILE");
    if (rank == 0 && mlggd_comm_unique_id(id) != MLGGD_OK) throw IoError(mlggd_last_error());
    mlggd_host::rendezvous(path ? path : "", world, rank, id, (double)env_int("MLGGD_RENDEZVOUS_TIMEOUT", 600));
}

// activation=sigmoid|relu; without the key, BPtrain_ReLU trains ReLU nets and every other name sigmoid ones
int activation_from_args(int argc, char **argv) {
    const char *slash = argc > 0 ? strrchr(argv[0], '/') : nullptr;
    const std::string prog = argc > 0 ? (slash ? slash + 1 : argv[0]) : "";
    int act = prog == "BPtrain_ReLU" ? MLGGD_ACT_RELU : MLGGD_ACT_SIGMOID;
    for (int a = 1; a < argc; a++) {
        if (strncmp(argv[a], "activation=", 11)) continue;
        const std::string v = argv[a] + 11;
        if (v == "sigmoid") act = MLGGD_ACT_SIGMOID;
        else if (v == "relu") act = MLGGD_ACT_RELU;
        else {
            fprintf(stderr, "activation=%s: must be sigmoid or relu\n", v.c_str());
            exit(1);
        }
    }
    return act;
}

}  // namespace

// Data-parallel runs only: RCCL collectives have no timeout, so a rank whose peer has died would sit in its next
// collective for ever.  The main thread bumps g_progress at every chunk / phase; if it stays unchanged for
// MLGGD_WATCHDOG_S seconds (default 900, 0 = off) this thread says where the rank was and ends the process with
// status 3, so that a launcher (or the batch system) sees a failure instead of a hang.
static std::atomic<long> g_progress{0};
static std::atomic<const char *> g_phase{"start"};
static void progress(const char *phase_name) {
    g_phase = phase_name;
    g_progress++;
}
static void watchdog_loop(int rank, int world, int timeout_s) {
    long seen = -1;
    double since = 0;
    for (;;) {
        std::this_thread::sleep_for(std::chrono::milliseconds(500));
        const long now = g_progress.load();
        if (now < 0) return;  // normal end of main
        if (now != seen) {
            seen = now;
            since = 0;
            continue;
        }
        since += 0.5;
        if (since >= timeout_s) {
            fprintf(stderr, "BPtrain watchdog: rank %d of %d made no progress for %d s in phase '%s' (step %ld); a peer has "
                            "probably died inside a collective -- giving up\n", rank, world, timeout_s, g_phase.load(), seen);
            fflush(stderr);
            _exit(3);
        }
    }
}

// MLGGD_TIMING=1: wall-clock of the phases on stderr (where does an epoch of the executable go?)
static double now_s() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}
static void phase(const char *name, double &t_last) {
    static const bool on = getenv("MLGGD_TIMING") != nullptr;
    const double t = now_s();
    if (on) fprintf(stderr, "[timing] %-28s %8.3f s\n", name, t - t_last);
    t_last = t;
}

int main(int argc, char *argv[]) {
    const double t_start = (double)time(NULL);
    double t_phase = now_s();
    const int activation = activation_from_args(argc, argv);
    const char *act_name = activation == MLGGD_ACT_RELU ? "relu" : "sigmoid";
    // BPtrain.cc:71: black on red when stdout is a terminal, as the reference prints it; plain text into pipes / logs
    printf(isatty(STDOUT_FILENO) ? "\033[41;30m--------activation functin is %s--------\033[0m\n"
                                 : "--------activation functin is %s--------\n", act_name);
    const int world = env_int("WORLD_SIZE", 1), rank = env_int("RANK", 0);
    const int local_rank = env_int("LOCAL_RANK", rank);
    Interface *io = new Interface;
    try {
        io->Initial(argc, argv, /*open_output=*/rank == 0);
        phase("arguments, norm, init weights", t_phase);
        WorkPara *p = io->para;
        const char *errmodel_fn = getenv("MLGGD_ERRMODEL");
        if (errmodel_fn && !*errmodel_fn) errmodel_fn = nullptr;
        std::vector<float> errmodel_betas;  // a bad grid ends the run here, not after the epoch
        if (errmodel_fn && rank == 0) errmodel_betas = mlggd_host::beta_grid(getenv("MLGGD_ERRMODEL_BETAS"));
        const char *gv_fn = getenv("MLGGD_GVFILE");
        if (gv_fn && !*gv_fn) gv_fn = nullptr;
        const char *shapes_fn = getenv("MLGGD_SHAPEFACTORS");
        if (shapes_fn && !*shapes_fn) shapes_fn = nullptr;
        std::vector<float> shapes;  // a bad file or a beta-norm run ends here, before anything is trained
        if (shapes_fn) {
            if (p->MLflag != 1)
                throw IoError(std::string("MLGGD_SHAPEFACTORS=") + shapes_fn + ": per-bin shape factors need MLflag=1, this run has MLflag=" +
                              std::to_string(p->MLflag));
            shapes.resize(p->layersizes[io->numlayers - 1]);
            std::string why;
            if (!mlggd_host::parse_shapefactors(shapes_fn, (int)shapes.size(), p->shapefactor, shapes.data(), &why))
                throw IoError("MLGGD_SHAPEFACTORS: " + why);
        }
        const char *asymmodel_fn = getenv("MLGGD_ASYMMODEL");
        if (asymmodel_fn && !*asymmodel_fn) asymmodel_fn = nullptr;
        std::vector<float> asymmodel_betas;  // a bad grid ends the run here, not after the epoch
        if (asymmodel_fn && rank == 0) asymmodel_betas = mlggd_host::beta_grid(getenv("MLGGD_ERRMODEL_BETAS"));
        const char *asym_fn = getenv("MLGGD_ASYMMETRY");
        if (asym_fn && !*asym_fn) asym_fn = nullptr;
        std::vector<float> skews;  // a bad file or a beta-norm run ends here, before anything is trained
        if (asym_fn) {
            if (p->MLflag != 1)
                throw IoError(std::string("MLGGD_ASYMMETRY=") + asym_fn + ": a skew per bin needs MLflag=1, this run has MLflag=" +
                              std::to_string(p->MLflag));
            skews.resize(p->layersizes[io->numlayers - 1]);
            std::string why;
            if (!mlggd_host::parse_asymmetry(asym_fn, (int)skews.size(), 1.0f, skews.data(), &why))
                throw IoError("MLGGD_ASYMMETRY: " + why);
        }
        // MLGGD_SCALE=learned: a bad value, a bad rate, a bad state file or a beta-norm run ends here, before anything is trained
        const char *scale_env = getenv("MLGGD_SCALE");
        if (scale_env && !*scale_env) scale_env = nullptr;
        const char *scale_fn = getenv("MLGGD_SCALE_FILE");
        if (scale_fn && !*scale_fn) scale_fn = nullptr;
        const bool scale_learned = scale_env && std::string(scale_env) == "learned";
        float scale_lrate = scale_rule::kLrate, scale_momentum = scale_rule::kMomentum, scale_vmax = scale_rule::kVmax;
        std::vector<float> scale_alpha, scale_velocity;  // the state MLGGD_SCALE_FILE held, empty: none
        long long scale_steps0 = 0;
        if (scale_env && !scale_learned && std::string(scale_env) != "alternating")
            throw IoError(std::string("MLGGD_SCALE=") + scale_env + ": must be learned or alternating");
        if (scale_fn && !scale_learned) throw IoError(std::string("MLGGD_SCALE_FILE=") + scale_fn + ": needs MLGGD_SCALE=learned");
        if (scale_learned) {
            if (p->MLflag != 1)
                throw IoError("MLGGD_SCALE=learned: a learned scale needs MLflag=1, this run has MLflag=" + std::to_string(p->MLflag));
            auto rate = [](const char *name, float *v) {
                const char *t = getenv(name);
                if (!t || !*t) return;
                char *end = nullptr;
                *v = strtof(t, &end);
                if (end == t || *end != 0) throw IoError(std::string(name) + "=" + t + ": not a number");
            };
            rate("MLGGD_SCALE_LRATE", &scale_lrate);
            rate("MLGGD_SCALE_MOMENTUM", &scale_momentum);
            rate("MLGGD_SCALE_VMAX", &scale_vmax);
            if (!scale_rule::valid(scale_rule::kLearned, scale_lrate, scale_momentum, scale_vmax))
                throw IoError("MLGGD_SCALE=learned: MLGGD_SCALE_LRATE must be finite and >= 0, MLGGD_SCALE_MOMENTUM in [0, 1), "
                              "MLGGD_SCALE_VMAX finite and > 0");
            FILE *have = scale_fn ? fopen(scale_fn, "r") : nullptr;  // no file yet: the first epoch seeds from its first minibatch
            if (have) {
                fclose(have);
                const int Dout = p->layersizes[io->numlayers - 1];
                scale_alpha.resize(Dout);
                scale_velocity.resize(Dout);
                std::string why;
                if (!mlggd_host::parse_scale_state(scale_fn, Dout, scale_alpha.data(), scale_velocity.data(), &why, &scale_steps0))
                    throw IoError("MLGGD_SCALE_FILE: " + why);
            }
        }
        // MLGGD_OPTIMIZER=adam: a bad value, a bad parameter, several ranks or a bad state file ends the run here, before
        // anything is trained
        const char *opt_env = getenv("MLGGD_OPTIMIZER");
        if (opt_env && !*opt_env) opt_env = nullptr;
        const char *opt_fn = getenv("MLGGD_OPT_FILE");
        if (opt_fn && !*opt_fn) opt_fn = nullptr;
        const bool adam = opt_env && std::string(opt_env) == "adam";
        float adam_b1 = adam_rule::kBeta1, adam_b2 = adam_rule::kBeta2, adam_eps = adam_rule::kEps;
        mlggd_host::OptState opt_state;  // what MLGGD_OPT_FILE held
        bool opt_restored = false;
        if (opt_env && !adam && std::string(opt_env) != "sgd") throw IoError(std::string("MLGGD_OPTIMIZER=") + opt_env + ": must be adam or sgd");
        if (opt_fn && !adam) throw IoError(std::string("MLGGD_OPT_FILE=") + opt_fn + ": needs MLGGD_OPTIMIZER=adam");
        if (adam) {
            if (world > 1)
                throw IoError("MLGGD_OPTIMIZER=adam: Adam runs on a single rank, this run has WORLD_SIZE=" + std::to_string(world));
            auto number = [](const char *name, float *v) {
                const char *t = getenv(name);
                if (!t || !*t) return;
                char *end = nullptr;
                *v = strtof(t, &end);
                if (end == t || *end != 0) throw IoError(std::string(name) + "=" + t + ": not a number");
            };
            number("MLGGD_ADAM_BETA1", &adam_b1);
            number("MLGGD_ADAM_BETA2", &adam_b2);
            number("MLGGD_ADAM_EPS", &adam_eps);
            if (!adam_rule::valid(adam_b1, adam_b2, adam_eps))
                throw IoError("MLGGD_OPTIMIZER=adam: MLGGD_ADAM_BETA1 and MLGGD_ADAM_BETA2 must lie in [0, 1), MLGGD_ADAM_EPS must be "
                              "finite and > 0");
            FILE *have = opt_fn ? fopen(opt_fn, "rb") : nullptr;  // no file yet: the first epoch starts from zero moments
            if (have) {
                fclose(have);
                std::string why;
                if (!mlggd_host::read_opt_state(opt_fn, p->layersizes, io->numlayers, &opt_state, &why))
                    throw IoError("MLGGD_OPT_FILE: " + why);
                opt_restored = true;
            }
        }
        // ---- train (BPtrain.cc:81-102).  The chunk plan and the fetch thread only touch host state, so the
        // first chunk is read while the engine initialises HIP and uploads the weights (the reference creates
        // BP_GPU first, BPtrain.cc:77-78, and reads the first chunk afterwards).
        io->get_pfile_info();
        io->get_chunk_info(p->train_sent_range);
        io->chunk_index.resize(io->total_chunks);
        for (unsigned i = 0; i < io->total_chunks; i++) io->chunk_index[i] = (int)i;
        io->GetRandIndex(io->chunk_index.data(), (int)io->total_chunks);

        Slot slot;
        std::string fetch_error;
        const bool frames = env_int("MLGGD_EXPANDED", 0) == 0;
        // page-locked chunk buffers: the per-chunk upload of ~200 MB runs at DMA speed instead of through
        // the runtime's staging copies
        // (allocated by the fetch thread, which has no current device of its own: the allocator names this
        // rank's device, so no rank pins its buffers through GPU 0's context)
        const int device = world > 1 ? local_rank : p->gpu_used;
        g_pinned_device = device;
        if (frames && env_int("MLGGD_PINNED", 1))
            io->set_buffer_allocator(
                [](size_t n) -> void * {
                    void *q = nullptr;
                    if (mlggd_alloc_pinned_on(g_pinned_device, n, &q) != MLGGD_OK) {
                        g_pinned_error = mlggd_last_error();
                        fprintf(stderr, "page-locked chunk buffer of %zu bytes: %s\n", n, g_pinned_error.c_str());
                        return nullptr;
                    }
                    return q;
                },
                [](void *q) { mlggd_free_pinned(q); });
        std::thread fetch(mlggd_host::fetch_loop, io, &slot, &fetch_error, frames, &g_stop_fetch, &g_pinned_error);
        struct FetchGuard {  // any exception from here on: stop and join the reader before unwinding
            std::thread &t;
            Slot &s;
            ~FetchGuard() {
                if (t.joinable()) {
                    g_stop_fetch = true;
                    s.set(false);
                    t.join();
                }
            }
        } fetch_guard{fetch, slot};
        phase("pfile headers, chunk plan", t_phase);

        std::thread watchdog;
        const int wd_s = env_int("MLGGD_WATCHDOG_S", 900);
        if (world > 1 && wd_s > 0) {
            watchdog = std::thread(watchdog_loop, rank, world, wd_s);
            watchdog.detach();
        }
        progress("engine + communicator");
        BP_GPU *net = new BP_GPU(p->init_randem_seed, device, io->numlayers, p->layersizes, p->bunchsize, p->lrate,
                                 p->momentum, p->weightcost, p->weights, p->bias, p->shapefactor, p->MLflag,
                                 p->dropoutflag, p->visible_omit, p->hid_omit, activation);
        if (world > 1) {
            unsigned char id[MLGGD_UNIQUE_ID_BYTES];
            exchange_id(world, rank, id);
            net->joinComm(id, world, rank);  // collective: returns once every rank has joined
            if (rank == 0) mlggd_host::rendezvous_cleanup(getenv("MLGGD_ID_FILE"), world);
        }
        if (shapes_fn) {
            net->setShapefactors(shapes.data());
            float lo = shapes[0], hi = shapes[0];
            double sum = 0;
            for (float b : shapes) {
                lo = b < lo ? b : lo;
                hi = b > hi ? b : hi;
                sum += b;
            }
            fprintf(stderr, "shape factors: %s, %zu bins, beta min %.9g max %.9g mean %.9g\n", shapes_fn, shapes.size(),
                    (double)lo, (double)hi, sum / (double)shapes.size());
        }
        if (asym_fn) {
            net->setAsymmetry(skews.data());
            float lo = skews[0], hi = skews[0];
            double sum = 0;
            for (float k : skews) {
                lo = k < lo ? k : lo;
                hi = k > hi ? k : hi;
                sum += k;
            }
            fprintf(stderr, "asymmetry: %s, %zu bins, kappa min %.9g max %.9g mean %.9g\n", asym_fn, skews.size(),
                    (double)lo, (double)hi, sum / (double)skews.size());
        }
        if (scale_learned) {
            net->setScaleLearned(scale_lrate, scale_momentum, scale_vmax);
            if (!scale_alpha.empty()) net->setScaleState(scale_alpha.data(), scale_velocity.data());
            fprintf(stderr, "learned scale: lrate %.9g momentum %.9g vmax %.9g, %s%s%s\n", (double)scale_lrate,
                    (double)scale_momentum, (double)scale_vmax, scale_alpha.empty() ? "every bin seeds from its first minibatch" : "state of ",
                    scale_alpha.empty() ? "" : scale_fn,
                    scale_alpha.empty() ? "" : (" after " + std::to_string(scale_steps0) + " steps").c_str());
        }
        // [L] pointer arrays with slot 0 unused over a state's vectors, as mlggd_get_weights takes them
        auto moment_ptrs = [&](std::vector<std::vector<float>> &g) {
            std::vector<float *> q((size_t)io->numlayers, nullptr);
            for (int l = 1; l < io->numlayers; l++) q[l] = g[l - 1].data();
            return q;
        };
        if (adam) {
            net->setOptimizerAdam(adam_b1, adam_b2, adam_eps);
            if (opt_restored) {
                // the file's own betas and eps describe the run that wrote it; this run's are the ones in effect
                std::vector<float *> mw = moment_ptrs(opt_state.m_w), vw = moment_ptrs(opt_state.v_w), mb = moment_ptrs(opt_state.m_b),
                                     vb = moment_ptrs(opt_state.v_b);
                net->setOptimizerState(mw.data(), vw.data(), mb.data(), vb.data(), opt_state.steps);
            }
            fprintf(stderr, "adam: beta1 %.9g beta2 %.9g eps %.9g, %s%s%s\n", (double)adam_b1, (double)adam_b2, (double)adam_eps,
                    opt_restored ? "state of " : "moments start from zero", opt_restored ? opt_fn : "",
                    opt_restored ? (" after " + std::to_string(opt_state.steps) + " steps").c_str() : "");
        }
        phase("engine (HIP init, upload)", t_phase);
        const int K0 = p->layersizes[0], D = p->layersizes[io->numlayers - 1], B = p->bunchsize;
        std::vector<float> loc_in, loc_targ;
        for (unsigned i = 0; i < io->total_chunks; i++) {
            progress("waiting for a chunk");
            if (!slot.wait(true)) break;  // the reader failed: its message is raised after the join below
            progress("training a chunk");
            io->logf("Starting chunk %d of %d containing %d samples.\n", i + 1, io->total_chunks, io->cur_chunk_samples);
            if (io->fp_log) fflush(io->fp_log);
            const int ns = io->cur_chunk_samples;
            if (frames) {
                const int *first = p->first_frame[1];
                std::vector<int> loc_first;
                int nloc = ns;
                if (world > 1) {  // this rank's rows of every complete global minibatch
                    const std::vector<int> rows = mlggd_host::rank_sample_rows(ns, B, world, rank);
                    loc_first.resize(rows.size());
                    for (size_t j = 0; j < rows.size(); j++) loc_first[j] = first[rows[j]];
                    first = loc_first.data();
                    nloc = (int)rows.size();
                }
                // no wait: the buffers are free once the chunk is on the device, and the next chunk's upload
                // overlaps these steps (the engine keeps two device buffer sets)
                net->train_frames(p->chunk_frames[1], p->fea_context, p->frames_in[1], p->frames_targ[1], nloc, first,
                                  p->targ_offset, /*wait=*/false);
            } else if (world == 1) {
                net->train(ns, p->indata[1], p->targ[1]);
            } else {
                // this rank's rows of every complete global minibatch, compacted
                const std::vector<int> rows = mlggd_host::rank_sample_rows(ns, B, world, rank);
                loc_in.resize(rows.size() * K0);
                loc_targ.resize(rows.size() * D);
                for (size_t j = 0; j < rows.size(); j++) {
                    memcpy(&loc_in[j * K0], p->indata[1] + (size_t)rows[j] * K0, (size_t)K0 * sizeof(float));
                    memcpy(&loc_targ[j * D], p->targ[1] + (size_t)rows[j] * D, (size_t)D * sizeof(float));
                }
                net->train((int)rows.size(), loc_in.data(), loc_targ.data());
            }
            slot.set(false);
        }
        fetch.join();
        if (!fetch_error.empty()) throw IoError(fetch_error);
        progress("final sync");
        net->sync();
        progress("weights / CV");
        phase("training chunks", t_phase);

        io->logf("Total cost time: %.1f s.\n", (double)time(NULL) - t_start);  // BPtrain.cc:104-105

        if (rank == 0) {
            printf("begin to write weights\n");
            net->returnWeights(p->weights, p->bias);
            io->Writeweights();
            printf("finish to write weights\n\n");
            // ---- the optimizer's state, for the next epoch's process
            if (adam && opt_fn) {
                mlggd_host::OptState st;
                st.layersizes.assign(p->layersizes, p->layersizes + io->numlayers);
                st.beta1 = adam_b1, st.beta2 = adam_b2, st.eps = adam_eps;
                for (int l = 1; l < io->numlayers; l++) {
                    const size_t kn = (size_t)p->layersizes[l - 1] * p->layersizes[l], n = (size_t)p->layersizes[l];
                    st.m_w.emplace_back(kn), st.v_w.emplace_back(kn), st.m_b.emplace_back(n), st.v_b.emplace_back(n);
                }
                std::vector<float *> mw = moment_ptrs(st.m_w), vw = moment_ptrs(st.v_w), mb = moment_ptrs(st.m_b), vb = moment_ptrs(st.v_b);
                net->getOptimizerState(mw.data(), vw.data(), mb.data(), vb.data());
                st.steps = net->optimizerSteps();
                std::string why;
                if (!mlggd_host::write_opt_state(opt_fn, st, &why)) throw IoError("MLGGD_OPT_FILE: " + why);
                printf("adam: %s written, %lld steps\n", opt_fn, st.steps);
            }
            phase("download + write weights", t_phase);

            // ---- CV (BPtrain.cc:112-140)
            printf("begin to CV\n");
            io->logf("Starting CV.\n");
            io->get_chunk_info_cv(p->cv_sent_range);
            float squared_err = 0.0f, dB_squared_err = 0.0f, likelihood = 0.0f;
            for (unsigned i = 0; i < io->cv_total_chunks; i++) {
                float sq = 0, ab = 0, ll = 0;
                int n;
                progress("cross validation");
                if (frames) {
                    if (i == 0) io->reserve_frame_buffers(io->cv_plan);  // the device is idle here (net->sync() above)
                    n = io->Readchunk_frames_cv((int)i);
                    net->CrossValidAll_frames(p->chunk_frames[0], p->fea_context, p->frames_in[0], p->frames_targ[0], n,
                                              p->first_frame[0], p->targ_offset, &sq, &ab, &ll);
                } else {
                    n = io->Readchunk_cv((int)i);
                    net->CrossValidAll(n, p->indata[0], p->targ[0], &sq, &ab, &ll);
                }
                printf("cur_chunk_samples=%d\n", n);
                squared_err += sq;
                dB_squared_err += ab;
                if (p->MLflag == 1) likelihood += ll;
            }
            const float cvacc = ((float)squared_err / io->cv_total_samples);
            io->logf("CV over. squared error: %f\n", cvacc);
            const float cvacc1 = ((float)dB_squared_err / io->cv_total_samples);
            io->logf("CV over. square root squared error: %f\n", cvacc1);
            if (p->MLflag == 1) {
                const float cvacc2 = ((float)likelihood / io->cv_total_samples);
                io->logf("CV2 over. CV log likelihood: %f\n", cvacc2);
            }
            if (io->fp_log) fflush(io->fp_log);
            phase("cross validation", t_phase);

            // ---- the learned scale's state, for the next epoch's process (every rank holds the same one)
            if (scale_learned && scale_fn) {
                std::vector<float> a(D), v(D);
                net->getScaleState(a.data(), v.data());
                const long long steps = scale_steps0 + net->scaleSteps();
                const mlggd_host::ScaleFileHeader h = {scale_lrate, scale_momentum, scale_vmax, steps};
                std::string why;
                if (!mlggd_host::write_scale_state(scale_fn, D, a.data(), v.data(), h, &why)) throw IoError("MLGGD_SCALE_FILE: " + why);
                printf("learned scale: %s written, %lld steps\n", scale_fn, steps);
            }

            // ---- the per-bin models of the CV set: one more pass over the CV chunks each, nothing of it reaches the log.
            // `stats` folds the chunk Readchunk*_cv left in the buffers into part ([rows][D], both chunk forms), the
            // parts are added, and `write` fits the total over n samples, writes `fn` and returns the shared value.
            auto cv_stats_pass = [&](const char *label, const char *var, const char *unavailable, const char *shared_what,
                                     const char *fn, size_t rows, auto stats, auto write) {
                if (!fn) return;
                if (p->dropoutflag != 0 || world > 1) {
                    printf("%s: %s %s; %s is not written\n", label, unavailable,
                           p->dropoutflag != 0 ? "with dropoutflag != 0" : "on a data-parallel run", fn);
                    return;
                }
                std::vector<double> total(rows * D, 0.0), part(total.size());
                int64_t n_total = 0;
                for (unsigned i = 0; i < io->cv_total_chunks; i++) {
                    progress(label);
                    const int n = frames ? io->Readchunk_frames_cv((int)i) : io->Readchunk_cv((int)i);
                    stats(n, part.data());
                    for (size_t j = 0; j < total.size(); j++) total[j] += part[j];
                    n_total += n;
                }
                if (n_total == 0) throw IoError(std::string(var) + ": the CV set has no samples, " + fn + " is not written");
                const double shared = write(n_total, total);
                printf("%s: %s written, %lld CV samples, %s %.9g\n", label, fn, (long long)n_total, shared_what, shared);
                phase(label, t_phase);
            };
            const int Ke = (int)errmodel_betas.size(), Ka = (int)asymmodel_betas.size();
            cv_stats_pass("error model", "MLGGD_ERRMODEL", "not available", "shared beta", errmodel_fn, 4 + Ke,
                [&](int n, double *part) {
                    if (frames)
                        net->ErrorStats_frames(p->chunk_frames[0], p->fea_context, p->frames_in[0], p->frames_targ[0], n,
                                               p->first_frame[0], p->targ_offset, Ke, errmodel_betas.data(), part);
                    else net->ErrorStats(n, p->indata[0], p->targ[0], Ke, errmodel_betas.data(), part);
                },
                [&](int64_t n, const std::vector<double> &total) {
                    return mlggd_host::write_error_model(errmodel_fn, D, n, errmodel_betas, total);
                });
            cv_stats_pass("asymmetric error model", "MLGGD_ASYMMODEL", "not available", "shared beta", asymmodel_fn, 2 * Ka,
                [&](int n, double *part) {
                    if (frames)
                        net->ErrorStatsSigned_frames(p->chunk_frames[0], p->fea_context, p->frames_in[0], p->frames_targ[0], n,
                                                     p->first_frame[0], p->targ_offset, Ka, asymmodel_betas.data(), part);
                    else net->ErrorStatsSigned(n, p->indata[0], p->targ[0], Ka, asymmodel_betas.data(), part);
                },
                [&](int64_t n, const std::vector<double> &total) {
                    return mlggd_host::write_asym_model(asymmodel_fn, D, n, asymmodel_betas, total);
                });
            cv_stats_pass("global variance", "MLGGD_GVFILE", "MLGGD_GVFILE is not available", "shared eta", gv_fn, 4,
                [&](int n, double *part) {
                    if (frames)
                        net->OutputStats_frames(p->chunk_frames[0], p->fea_context, p->frames_in[0], p->frames_targ[0], n,
                                                p->first_frame[0], p->targ_offset, part);
                    else net->OutputStats(n, p->indata[0], p->targ[0], part);
                },
                [&](int64_t n, const std::vector<double> &total) {
                    return (double)mlggd_host::write_gv_file(gv_fn, D, n, total);
                });
        }
        printf("all finish!\n");
        g_progress = -1000000;  // the watchdog leaves
        delete net;
        delete io;
        phase("teardown", t_phase);
    } catch (const std::exception &e) {
        // the reference writes the message to the log and exit(0)s (e.g. Interface.cc:320,325,451);
        // same message, non-zero status
        io->logf("%s\n", e.what());
        if (io->fp_log) fflush(io->fp_log);
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
