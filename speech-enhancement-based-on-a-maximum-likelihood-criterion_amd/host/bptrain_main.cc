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
// Options (new, all opt-in): everything the environment selects -- the per-bin models written after the epoch, per-bin
// shapes and skews, the learned scale, Adam -- is read and checked in one place, train_options.cc, and described
// beside its field in train_options.h; this file applies it.
//
// Activation (new): activation=sigmoid|relu selects the hidden units (mlggd_config.activation).  Without the key the
// program's own name decides: installed as BPtrain_ReLU -- the same program -- it trains rectified-linear nets, under
// any other name sigmoid ones, so a finetune.pl edited only in its $exe line trains a ReLU net.  Any other value ends
// the run before a file or a device is opened.  The banner line names the choice; the log file does not change.
//
// Data parallel (new): when WORLD_SIZE > 1 (torchrun-style env: RANK,
// LOCAL_RANK, WORLD_SIZE; MLGGD_ID_FILE names a file on a shared filesystem used to hand the
// RCCL unique id from rank 0 to the others) every rank reads the same chunks with the same
// seed and trains rows [rank*bunchsize,(rank+1)*bunchsize) of each global minibatch of
// WORLD_SIZE*bunchsize samples; rank 0 alone writes the log, the weights and runs CV.
#include <chrono>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
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
#include "optfile.h"
#include "prefetch.h"
#include "train_options.h"
#include "trainer_io.h"

using mlggd_host::Interface;
using mlggd_host::IoError;
using mlggd_host::TrainOptions;
using mlggd_host::WorkPara;

namespace {

std::atomic<bool> g_stop_fetch{false};  // set when the trainer gives up before consuming every chunk
int g_pinned_device = 0;                // device whose context owns the page-locked chunk buffers
std::string g_pinned_error;             // engine's message when a page-locked allocation failed (fetch thread only)

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

// Data-parallel runs only: RCCL collectives have no timeout, so a rank whose peer has died would sit in its next
// collective for ever.  The main thread bumps g_progress at every chunk / phase; if it stays unchanged for
// MLGGD_WATCHDOG_S seconds (default 900, 0 = off) this thread says where the rank was and ends the process with
// status 3, so that a launcher (or the batch system) sees a failure instead of a hang.
std::atomic<long> g_progress{0};
std::atomic<const char *> g_phase{"start"};
void progress(const char *phase_name) {
    g_phase = phase_name;
    g_progress++;
}
void watchdog_loop(int rank, int world, int timeout_s) {
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
bool g_timing = false;
double g_t_phase = 0;
double now_s() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}
void phase(const char *name) {
    const double t = now_s();
    if (g_timing) fprintf(stderr, "[timing] %-28s %8.3f s\n", name, t - g_t_phase);
    g_t_phase = t;
}

// what the steps of main() share
struct Trainer {
    Interface *io;
    WorkPara *p;
    int activation;
    TrainOptions opt;
    int device = 0;
    BP_GPU *net = nullptr;
};

// The reader thread and its hand-off.  Any exception while it runs: it is stopped and joined before unwinding goes on.
struct Fetch {
    mlggd_host::Slot slot;
    std::string error;
    std::thread thread;
    ~Fetch() {
        if (thread.joinable()) {
            g_stop_fetch = true;
            slot.set(false);
            thread.join();
        }
    }
};

// ---- the chunk plan and the reader (BPtrain.cc:81-102).  Both only touch host state, so the first chunk is read while
// the engine initialises HIP and uploads the weights (the reference creates BP_GPU first, BPtrain.cc:77-78, and reads
// the first chunk afterwards).
void plan_and_start_fetch(Trainer &t, Fetch &fetch) {
    Interface *io = t.io;
    io->get_pfile_info();
    io->get_chunk_info(t.p->train_sent_range);
    io->chunk_index.resize(io->total_chunks);
    for (unsigned i = 0; i < io->total_chunks; i++) io->chunk_index[i] = (int)i;
    io->GetRandIndex(io->chunk_index.data(), (int)io->total_chunks);
    // page-locked chunk buffers: the per-chunk upload of ~200 MB runs at DMA speed instead of through
    // the runtime's staging copies
    // (allocated by the fetch thread, which has no current device of its own: the allocator names this
    // rank's device, so no rank pins its buffers through GPU 0's context)
    t.device = t.opt.world > 1 ? t.opt.local_rank : t.p->gpu_used;
    g_pinned_device = t.device;
    if (t.opt.frames && t.opt.pinned)
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
    fetch.thread = std::thread(mlggd_host::fetch_loop, io, &fetch.slot, &fetch.error, t.opt.frames, &g_stop_fetch, &g_pinned_error);
}

void start_engine_and_communicator(Trainer &t) {
    const TrainOptions &o = t.opt;
    WorkPara *p = t.p;
    if (o.world > 1 && o.watchdog_s > 0) std::thread(watchdog_loop, o.rank, o.world, o.watchdog_s).detach();
    progress("engine + communicator");
    t.net = new BP_GPU(p->init_randem_seed, t.device, t.io->numlayers, p->layersizes, p->bunchsize, p->lrate, p->momentum,
                       p->weightcost, p->weights, p->bias, p->shapefactor, p->MLflag, p->dropoutflag, p->visible_omit,
                       p->hid_omit, t.activation);
    if (o.world > 1) {
        // rank 0 creates the RCCL id and hands it to the other ranks through MLGGD_ID_FILE (dp_launch.h: a handshake
        // with per-launch nonces, so a file left by an earlier epoch's launch is never accepted)
        static_assert(MLGGD_UNIQUE_ID_BYTES == mlggd_host::kUniqueIdBytes, "id size");
        unsigned char id[MLGGD_UNIQUE_ID_BYTES];
        if (o.rank == 0 && mlggd_comm_unique_id(id) != MLGGD_OK) throw IoError(mlggd_last_error());
        mlggd_host::rendezvous(o.id_file, o.world, o.rank, id, (double)o.rendezvous_timeout);
        t.net->joinComm(id, o.world, o.rank);  // collective: returns once every rank has joined
        if (o.rank == 0) mlggd_host::rendezvous_cleanup(o.id_file, o.world);
    }
}

// one stderr line on a per-bin vector: the file it came from, its minimum, maximum and mean
void report_bins(const char *label, const char *symbol, const std::string &fn, const std::vector<float> &v) {
    float lo = v[0], hi = v[0];
    double sum = 0;
    for (float x : v) {
        lo = x < lo ? x : lo;
        hi = x > hi ? x : hi;
        sum += x;
    }
    fprintf(stderr, "%s: %s, %zu bins, %s min %.9g max %.9g mean %.9g\n", label, fn.c_str(), v.size(), symbol, (double)lo,
            (double)hi, sum / (double)v.size());
}

// [L] pointer arrays with slot 0 unused over a state's vectors, as mlggd_get_weights takes them
std::vector<float *> moment_ptrs(std::vector<std::vector<float>> &g) {
    std::vector<float *> q(g.size() + 1, nullptr);
    for (size_t l = 1; l <= g.size(); l++) q[l] = g[l - 1].data();
    return q;
}

// what the options set on the engine before the first chunk, one stderr line each (the options are not const: the
// shim's setOptimizerState takes float ** like its getter)
void apply_train_options(BP_GPU &net, TrainOptions &o) {
    if (!o.shapes_fn.empty()) {
        net.setShapefactors(o.shapes.data());
        report_bins("shape factors", "beta", o.shapes_fn, o.shapes);
    }
    if (!o.asym_fn.empty()) {
        net.setAsymmetry(o.skews.data());
        report_bins("asymmetry", "kappa", o.asym_fn, o.skews);
    }
    if (o.scale_learned) {
        const bool restored = !o.scale_alpha.empty();
        net.setScaleLearned(o.scale_lrate, o.scale_momentum, o.scale_vmax);
        if (restored) net.setScaleState(o.scale_alpha.data(), o.scale_velocity.data());
        fprintf(stderr, "learned scale: lrate %.9g momentum %.9g vmax %.9g, %s%s%s\n", (double)o.scale_lrate, (double)o.scale_momentum,
                (double)o.scale_vmax, restored ? "state of " : "every bin seeds from its first minibatch",
                restored ? o.scale_fn.c_str() : "", restored ? (" after " + std::to_string(o.scale_steps0) + " steps").c_str() : "");
    }
    if (o.adam) {
        mlggd_host::OptState &st = o.opt_state;
        net.setOptimizerAdam(o.adam_beta1, o.adam_beta2, o.adam_eps);
        // the file's own betas and eps describe the run that wrote it; this run's are the ones in effect
        if (o.opt_restored)
            net.setOptimizerState(moment_ptrs(st.m_w).data(), moment_ptrs(st.v_w).data(), moment_ptrs(st.m_b).data(),
                                  moment_ptrs(st.v_b).data(), st.steps);
        fprintf(stderr, "adam: beta1 %.9g beta2 %.9g eps %.9g, %s%s%s\n", (double)o.adam_beta1, (double)o.adam_beta2, (double)o.adam_eps,
                o.opt_restored ? "state of " : "moments start from zero", o.opt_restored ? o.opt_fn.c_str() : "",
                o.opt_restored ? (" after " + std::to_string(st.steps) + " steps").c_str() : "");
    }
}

void train_chunks(Trainer &t, Fetch &fetch) {
    Interface *io = t.io;
    WorkPara *p = t.p;
    BP_GPU *net = t.net;
    const int world = t.opt.world, rank = t.opt.rank;
    const int K0 = p->layersizes[0], D = p->layersizes[io->numlayers - 1], B = p->bunchsize;
    std::vector<float> loc_in, loc_targ;
    for (unsigned i = 0; i < io->total_chunks; i++) {
        progress("waiting for a chunk");
        if (!fetch.slot.wait(true)) break;  // the reader failed: its message is raised after the join below
        progress("training a chunk");
        io->logf("Starting chunk %d of %d containing %d samples.\n", i + 1, io->total_chunks, io->cur_chunk_samples);
        if (io->fp_log) fflush(io->fp_log);
        const int ns = io->cur_chunk_samples;
        if (t.opt.frames) {
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
        fetch.slot.set(false);
    }
    fetch.thread.join();
    if (!fetch.error.empty()) throw IoError(fetch.error);
    progress("final sync");
    net->sync();
    progress("weights / CV");
}

void write_weights(Trainer &t) {
    printf("begin to write weights\n");
    t.net->returnWeights(t.p->weights, t.p->bias);
    t.io->Writeweights();
    printf("finish to write weights\n\n");
}

// ---- the optimizer's state, for the next epoch's process
void write_optimizer_state(Trainer &t) {
    const TrainOptions &o = t.opt;
    if (!o.adam || o.opt_fn.empty()) return;
    const int *ls = t.p->layersizes;
    mlggd_host::OptState st;
    st.layersizes.assign(ls, ls + t.io->numlayers);
    st.beta1 = o.adam_beta1, st.beta2 = o.adam_beta2, st.eps = o.adam_eps;
    for (int l = 1; l < t.io->numlayers; l++) {
        const size_t kn = (size_t)ls[l - 1] * ls[l], n = (size_t)ls[l];
        st.m_w.emplace_back(kn), st.v_w.emplace_back(kn), st.m_b.emplace_back(n), st.v_b.emplace_back(n);
    }
    t.net->getOptimizerState(moment_ptrs(st.m_w).data(), moment_ptrs(st.v_w).data(), moment_ptrs(st.m_b).data(),
                             moment_ptrs(st.v_b).data());
    st.steps = t.net->optimizerSteps();
    std::string why;
    if (!mlggd_host::write_opt_state(o.opt_fn, st, &why)) throw IoError("MLGGD_OPT_FILE: " + why);
    printf("adam: %s written, %lld steps\n", o.opt_fn.c_str(), st.steps);
}

// ---- CV (BPtrain.cc:112-140) and the three log lines
void cross_validate(Trainer &t) {
    Interface *io = t.io;
    WorkPara *p = t.p;
    printf("begin to CV\n");
    io->logf("Starting CV.\n");
    io->get_chunk_info_cv(p->cv_sent_range);
    float squared_err = 0.0f, dB_squared_err = 0.0f, likelihood = 0.0f;
    for (unsigned i = 0; i < io->cv_total_chunks; i++) {
        float sq = 0, ab = 0, ll = 0;
        int n;
        progress("cross validation");
        if (t.opt.frames) {
            if (i == 0) io->reserve_frame_buffers(io->cv_plan);  // the device is idle here (net->sync() above)
            n = io->Readchunk_frames_cv((int)i);
            t.net->CrossValidAll_frames(p->chunk_frames[0], p->fea_context, p->frames_in[0], p->frames_targ[0], n,
                                        p->first_frame[0], p->targ_offset, &sq, &ab, &ll);
        } else {
            n = io->Readchunk_cv((int)i);
            t.net->CrossValidAll(n, p->indata[0], p->targ[0], &sq, &ab, &ll);
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
}

// ---- the learned scale's state, for the next epoch's process (every rank holds the same one)
void write_scale_state(Trainer &t) {
    const TrainOptions &o = t.opt;
    if (!o.scale_learned || o.scale_fn.empty()) return;
    const int D = t.p->layersizes[t.io->numlayers - 1];
    std::vector<float> a(D), v(D);
    t.net->getScaleState(a.data(), v.data());
    const long long steps = o.scale_steps0 + t.net->scaleSteps();
    const mlggd_host::ScaleFileHeader h = {o.scale_lrate, o.scale_momentum, o.scale_vmax, steps};
    std::string why;
    if (!mlggd_host::write_scale_state(o.scale_fn, D, a.data(), v.data(), h, &why)) throw IoError("MLGGD_SCALE_FILE: " + why);
    printf("learned scale: %s written, %lld steps\n", o.scale_fn.c_str(), steps);
}

// ---- a per-bin model of the CV set: one more pass over the CV chunks, nothing of it reaches the log.
// `stats` folds the chunk Readchunk*_cv left in the buffers into part ([rows][D], both chunk forms), the
// parts are added, and `write` fits the total over n samples, writes `fn` and returns the shared value.
template <class Stats, class Write>
void cv_stats_pass(Trainer &t, const char *label, const char *var, const char *unavailable, const char *shared_what,
                   const std::string &fn, size_t rows, Stats stats, Write write) {
    Interface *io = t.io;
    if (fn.empty()) return;
    if (t.p->dropoutflag != 0 || t.opt.world > 1) {
        printf("%s: %s %s; %s is not written\n", label, unavailable,
               t.p->dropoutflag != 0 ? "with dropoutflag != 0" : "on a data-parallel run", fn.c_str());
        return;
    }
    std::vector<double> total(rows * t.p->layersizes[io->numlayers - 1], 0.0), part(total.size());
    int64_t n_total = 0;
    for (unsigned i = 0; i < io->cv_total_chunks; i++) {
        progress(label);
        const int n = t.opt.frames ? io->Readchunk_frames_cv((int)i) : io->Readchunk_cv((int)i);
        stats(n, part.data());
        for (size_t j = 0; j < total.size(); j++) total[j] += part[j];
        n_total += n;
    }
    if (n_total == 0) throw IoError(std::string(var) + ": the CV set has no samples, " + fn + " is not written");
    const double shared = write(n_total, total);
    printf("%s: %s written, %lld CV samples, %s %.9g\n", label, fn.c_str(), (long long)n_total, shared_what, shared);
    phase(label);
}

void write_cv_models(Trainer &t) {
    const TrainOptions &o = t.opt;
    WorkPara *p = t.p;
    BP_GPU *net = t.net;
    const bool frames = o.frames;
    const int D = p->layersizes[t.io->numlayers - 1], K = (int)o.model_betas.size();
    const float *betas = o.model_betas.data();
    cv_stats_pass(t, "error model", "MLGGD_ERRMODEL", "not available", "shared beta", o.errmodel_fn, 4 + K,
        [&](int n, double *part) {
            if (frames)
                net->ErrorStats_frames(p->chunk_frames[0], p->fea_context, p->frames_in[0], p->frames_targ[0], n,
                                       p->first_frame[0], p->targ_offset, K, betas, part);
            else net->ErrorStats(n, p->indata[0], p->targ[0], K, betas, part);
        },
        [&](int64_t n, const std::vector<double> &total) {
            return mlggd_host::write_error_model(o.errmodel_fn, D, n, o.model_betas, total);
        });
    cv_stats_pass(t, "asymmetric error model", "MLGGD_ASYMMODEL", "not available", "shared beta", o.asymmodel_fn, 2 * K,
        [&](int n, double *part) {
            if (frames)
                net->ErrorStatsSigned_frames(p->chunk_frames[0], p->fea_context, p->frames_in[0], p->frames_targ[0], n,
                                             p->first_frame[0], p->targ_offset, K, betas, part);
            else net->ErrorStatsSigned(n, p->indata[0], p->targ[0], K, betas, part);
        },
        [&](int64_t n, const std::vector<double> &total) {
            return mlggd_host::write_asym_model(o.asymmodel_fn, D, n, o.model_betas, total);
        });
    cv_stats_pass(t, "global variance", "MLGGD_GVFILE", "MLGGD_GVFILE is not available", "shared eta", o.gv_fn, 4,
        [&](int n, double *part) {
            if (frames)
                net->OutputStats_frames(p->chunk_frames[0], p->fea_context, p->frames_in[0], p->frames_targ[0], n,
                                        p->first_frame[0], p->targ_offset, part);
            else net->OutputStats(n, p->indata[0], p->targ[0], part);
        },
        [&](int64_t n, const std::vector<double> &total) { return (double)mlggd_host::write_gv_file(o.gv_fn, D, n, total); });
}

}  // namespace

int main(int argc, char *argv[]) {
    const double t_start = (double)time(NULL);
    g_t_phase = now_s();
    const int activation = activation_from_args(argc, argv);
    // BPtrain.cc:71: black on red when stdout is a terminal, as the reference prints it; plain text into pipes / logs
    printf(isatty(STDOUT_FILENO) ? "\033[41;30m--------activation functin is %s--------\033[0m\n"
                                 : "--------activation functin is %s--------\n", activation == MLGGD_ACT_RELU ? "relu" : "sigmoid");
    const mlggd_host::LaunchEnv launch = mlggd_host::read_launch_env();
    g_timing = launch.timing;
    Interface *io = new Interface;
    try {
        io->Initial(argc, argv, /*open_output=*/launch.rank == 0);
        phase("arguments, norm, init weights");
        Trainer t{io, io->para, activation, mlggd_host::read_train_options(*io->para, io->numlayers)};
        Fetch fetch;  // from here on any exception stops and joins the reader before it leaves
        plan_and_start_fetch(t, fetch);
        phase("pfile headers, chunk plan");
        start_engine_and_communicator(t);
        apply_train_options(*t.net, t.opt);
        phase("engine (HIP init, upload)");
        train_chunks(t, fetch);
        phase("training chunks");
        io->logf("Total cost time: %.1f s.\n", (double)time(NULL) - t_start);  // BPtrain.cc:104-105
        if (t.opt.rank == 0) {
            write_weights(t);
            write_optimizer_state(t);
            phase("download + write weights");
            cross_validate(t);
            phase("cross validation");
            write_scale_state(t);
            write_cv_models(t);
        }
        printf("all finish!\n");
        g_progress = -1000000;  // the watchdog leaves
        delete t.net;
        delete io;
        phase("teardown");
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
