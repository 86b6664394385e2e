// engine.hip -- host side of the MI355X training engine behind the C-ABI of include/mlggd.h.
//
// Mirrors what the reference's class BP_GPU does on the host (Train_code_ML_GGD/BP_GPU.cu):
// device workspace (BP_WorkSpace, BP_GPU.h:17-43), chunk upload, the bunch loop, CV metric
// accumulation and weight read-back -- re-designed for one HIP stream of fused gfx950 kernels
// (kernels.hip.h) instead of ~50 launches + cuBLAS on two racing streams.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mlggd.h"
#include "../host/errmodel.h"  // parse_shapefactors: one file format, one reader and one writer
#include "../host/gvfile.h"    // parse_gv: the same for the global variance file
#include "../host/asymfile.h"  // parse_asymmetry: the same for the asymmetric error model's file
#include "../host/scalefile.h"  // parse_scale_state / write_scale_state: the learned scale's state file
#include "../host/optfile.h"    // read_opt_state / write_opt_state: the optimizer's state file
#include "kernels.hip.h"
#include "spectral.hip.h"
#include "score.hip.h"
#include "stoi.hip.h"
#include "stoi_rule.h"
#include "live.hip.h"
#include "live_rule.h"
#include "colstats.hip.h"
#include "gv_rule.h"
#include "mask_rule.h"
#include "mix.hip.h"
#include "mix_rule.h"
#include "nat_rule.h"
#include "rbm_rule.h"
#include "devbuf.h"

// ------------------------------------------------------------------ errors
static thread_local char g_err[1024] = "";
static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(MLGGD_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
#define CHK(expr)                 \
    do {                          \
        int _rc = (expr);         \
        if (_rc != MLGGD_OK) return _rc; \
    } while (0)
// a check of a *_rule.h header (host only, no fail()): 0, or -1 with its message written to RULE_MSG
static thread_local char g_rule_msg[512];
#define RULE_MSG g_rule_msg, sizeof(g_rule_msg)
#define RULE(expr) CHK((expr) != 0 ? fail(MLGGD_ERR_ARG, "%s", g_rule_msg) : MLGGD_OK)

static inline int ceil32(int x) { return (x + 31) & ~31; }

// ------------------------------------------------------------------ RCCL (loaded on demand)
// Only the data-parallel path needs RCCL; it is dlopen'ed at mlggd_comm_init so a single-GPU process never maps
// it.  The function-pointer types are taken from rccl.h itself (decltype of the declarations; the header is only
// compiled against, nothing is linked), so a signature change in the library breaks the build, not a multi-GPU run.
#include <rccl/rccl.h>
static_assert(sizeof(ncclUniqueId) == MLGGD_UNIQUE_ID_BYTES, "include/mlggd.h MLGGD_UNIQUE_ID_BYTES != sizeof(ncclUniqueId)");
typedef ncclUniqueId RcclUniqueId;
typedef ncclComm_t RcclComm;
struct RcclApi {
    void *lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllReduce) AllReduce_ = nullptr;
    decltype(&ncclAllGather) AllGather_ = nullptr;
    decltype(&ncclReduceScatter) ReduceScatter_ = nullptr;
    decltype(&ncclSend) Send_ = nullptr;  // optional: the all-to-all form of the sharded update
    decltype(&ncclRecv) Recv_ = nullptr;
    decltype(&ncclCommSplit) CommSplit = nullptr;        // optional: MLGGD_DP_STAT_COMM
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString_ = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;        // optional: mlggd_comm_info
    decltype(&ncclCommUserRank) CommUserRank = nullptr;  // optional: mlggd_comm_info
    // fp32 sum / fp32 gather, the only forms the engine uses (the int arguments of the call sites are ignored: they
    // date from the hand-written prototypes and are kept so the call sites read like the NCCL API)
    int AllReduce(const void *s, void *r, size_t n, int, int, RcclComm c, hipStream_t st) const {
        return (int)AllReduce_(s, r, n, ncclFloat32, ncclSum, c, st);
    }
    int AllGather(const void *s, void *r, size_t n, int, RcclComm c, hipStream_t st) const {
        return (int)AllGather_(s, r, n, ncclFloat32, c, st);
    }
    // r receives this rank's block of n floats of the sum over the ranks of the world*n floats at s
    int ReduceScatter(const void *s, void *r, size_t n, RcclComm c, hipStream_t st) const {
        return (int)ReduceScatter_(s, r, n, ncclFloat32, ncclSum, c, st);
    }
    const char *GetErrorString(int rc) const { return GetErrorString_ ? GetErrorString_((ncclResult_t)rc) : "rccl error"; }
};
static RcclApi g_rccl;
static int rccl_load() {
    if (g_rccl.lib) return MLGGD_OK;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *lib = nullptr;
    for (const char *n : names) {
        lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (lib) break;
    }
    if (!lib) return fail(MLGGD_ERR_COMM, "cannot dlopen librccl: %s", dlerror());
    g_rccl.GetUniqueId = (decltype(&ncclGetUniqueId))dlsym(lib, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(&ncclCommInitRank))dlsym(lib, "ncclCommInitRank");
    g_rccl.AllReduce_ = (decltype(&ncclAllReduce))dlsym(lib, "ncclAllReduce");
    g_rccl.AllGather_ = (decltype(&ncclAllGather))dlsym(lib, "ncclAllGather");
    g_rccl.ReduceScatter_ = (decltype(&ncclReduceScatter))dlsym(lib, "ncclReduceScatter");
    g_rccl.CommSplit = (decltype(&ncclCommSplit))dlsym(lib, "ncclCommSplit");
    g_rccl.Send_ = (decltype(&ncclSend))dlsym(lib, "ncclSend");
    g_rccl.Recv_ = (decltype(&ncclRecv))dlsym(lib, "ncclRecv");
    g_rccl.CommDestroy = (decltype(&ncclCommDestroy))dlsym(lib, "ncclCommDestroy");
    g_rccl.GetErrorString_ = (decltype(&ncclGetErrorString))dlsym(lib, "ncclGetErrorString");
    g_rccl.GroupStart = (decltype(&ncclGroupStart))dlsym(lib, "ncclGroupStart");
    g_rccl.GroupEnd = (decltype(&ncclGroupEnd))dlsym(lib, "ncclGroupEnd");
    g_rccl.CommCount = (decltype(&ncclCommCount))dlsym(lib, "ncclCommCount");
    g_rccl.CommUserRank = (decltype(&ncclCommUserRank))dlsym(lib, "ncclCommUserRank");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce_ || !g_rccl.AllGather_ || !g_rccl.ReduceScatter_ || !g_rccl.CommDestroy ||
        !g_rccl.GroupStart || !g_rccl.GroupEnd)
        return fail(MLGGD_ERR_COMM, "librccl is missing required symbols");
    g_rccl.lib = lib;
    return MLGGD_OK;
}
#define NCCLCHK(expr)                                                                              \
    do {                                                                                           \
        int _r = (expr);                                                                           \
        if (_r != 0)                                                                               \
            return fail(MLGGD_ERR_COMM, "%s failed: %s", #expr, g_rccl.GetErrorString(_r));        \
    } while (0)

// ------------------------------------------------------------------ ROCTX ranges (loaded on demand)
// MLGGD_ROCTX=1: the phases of every training step (forward, loss, backward, weight update, exchange) are bracketed
// with roctxRangePush / Pop so that `rocprofv3 --marker-trace --kernel-trace` shows them around the kernels they
// enqueue (the reference has no profiling hooks at all, BP_GPU.h:8-16 is an unused macro).
// rocprofv3's own roctx library is tried first, the roctracer one second; off (and never loaded) by default.
struct RoctxApi {
    bool tried = false, on = false;
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
};
static RoctxApi g_roctx;
static void roctx_load() {
    if (g_roctx.tried) return;
    g_roctx.tried = true;
    const char *v = getenv("MLGGD_ROCTX");
    if (!v || !atoi(v)) return;
    for (const char *n : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
        void *lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (!lib) continue;
        g_roctx.push = (int (*)(const char *))dlsym(lib, "roctxRangePushA");
        g_roctx.pop = (int (*)())dlsym(lib, "roctxRangePop");
        if (g_roctx.push && g_roctx.pop) {
            g_roctx.on = true;
            return;
        }
    }
    fprintf(stderr, "mlggd: MLGGD_ROCTX is set but no roctx library could be loaded\n");
}
struct RoctxRange {  // scope guard; a no-op unless MLGGD_ROCTX=1
    bool on;
    explicit RoctxRange(const char *name) : on(g_roctx.on) {
        if (on) g_roctx.push(name);
    }
    ~RoctxRange() {
        if (on) g_roctx.pop();
    }
};

// ------------------------------------------------------------------ engine state
enum KernelClass { KC_TRANSPOSE = 0, KC_FWD, KC_LOSS, KC_DX, KC_DW, KC_UPDATE, KC_COUNT };
static const char *kKernelClassName[KC_COUNT] = {"transpose", "fwd", "loss", "dx", "dw", "update"};

struct mlggd_engine {
    DevBufStats bufs;  // of every DevBuf below and of the engine's live groups; declared first: destroyed last
    mlggd_config cfg;
    int L = 0;
    int ls[MLGGD_MAXLAYER] = {0};   // true units
    int lsp[MLGGD_MAXLAYER] = {0};  // padded to 32
    int B = 0, Bp = 0, D = 0, Dp = 0, K0 = 0;
    int device = 0;
    hipStream_t stream = nullptr, comm_stream = nullptr;

    float *W[MLGGD_MAXLAYER] = {0}, *dW[MLGGD_MAXLAYER] = {0};
    float *bias[MLGGD_MAXLAYER] = {0}, *dbias[MLGGD_MAXLAYER] = {0};
    float *G[MLGGD_MAXLAYER] = {0}, *gb[MLGGD_MAXLAYER] = {0};
    float *gb_all = nullptr;
    size_t gb_all_count = 0;
    // one-GPU emulation of a world (mlggd_debug_fake_world): sums over the emulated ranks 0..world-2
    float *Gpre[MLGGD_MAXLAYER] = {0}, *gbpre = nullptr, *colsum_tot = nullptr;
    float *Yt[MLGGD_MAXLAYER] = {0}, *Y[MLGGD_MAXLAYER] = {0};
    float *dEdXt[MLGGD_MAXLAYER] = {0}, *dEdX[MLGGD_MAXLAYER] = {0};
    float *slab = nullptr, *outT = nullptr, *eT = nullptr, *pT = nullptr, *colsum = nullptr, *scalefactor = nullptr;
    int S_out = 1;
    // mlggd_set_shapefactors: one shape per output bin.  betas_dev [Dp] (pads 1.0) exists from the first set on and is
    // only read while per_bin is on; betas_host [D] is what mlggd_get_shapefactors returns and the CV sums use.
    bool per_bin = false;
    float *betas_dev = nullptr;
    std::vector<float> betas_host;
    // mlggd_set_asymmetry: one skew per output bin (asym_rule.h).  kappas_dev [Dp] (pads 1.0) and asym_betas_dev [Dp]
    // (cfg.shapefactor, pads 1.0: the shapes the _asym kernels read on an engine without a shape vector) exist from the
    // first set on and are only read while asym is on; kappas_host [D] is what mlggd_get_asymmetry returns.
    bool asym = false;
    DevBuf<float> kappas_dev, asym_betas_dev;
    std::vector<float> kappas_host;
    // mlggd_set_scale_mode: the scale as a learned parameter (scale_rule.h).  scale_state is [2 copies][alpha, v][Dp]
    // (pads 0), allocated when the mode is first switched on; a step's loss launches read copy scale_cur and write the
    // other one, and run_step swaps them once its last loss launch is enqueued.  scale_steps counts those swaps.
    int scale_mode = MLGGD_SCALE_ALTERNATING;
    float scale_lrate = scale_rule::kLrate, scale_momentum = scale_rule::kMomentum, scale_vmax = scale_rule::kVmax;
    DevBuf<float> scale_state;
    int scale_cur = 0;
    long long scale_steps = 0;
    // mlggd_set_optimizer: Adam beside SGD with momentum (adam_rule.h).  Entering the mode allocates, per layer, the two
    // moments of the padded weight matrix and of the bias (zero pads that stay zero) and the gradient buffers G_l / gb_l
    // the unfused dW launches write (the all-reduce exchange's own, which a single-device engine does not have); a step
    // then ends with one k_adam_apply launch over all of them.  adam_steps counts the updates, adam_prod holds
    // beta1^steps and beta2^steps as running products in double.  Nothing here exists on an engine that never entered it.
    int opt_kind = MLGGD_OPT_SGD;
    float adam_b1 = adam_rule::kBeta1, adam_b2 = adam_rule::kBeta2, adam_eps = adam_rule::kEps;
    long long adam_steps = 0;
    adam_rule::Products adam_prod;
    DevBuf<float> adam_mw[MLGGD_MAXLAYER], adam_vw[MLGGD_MAXLAYER], adam_mb[MLGGD_MAXLAYER], adam_vb[MLGGD_MAXLAYER];
    DevBuf<float> adam_G[MLGGD_MAXLAYER], adam_gb;
    DevBuf<float> chunk_in, chunk_targ, chunk_out;
    // CV metrics: 0 = outputs copied back, host fp32 accumulation in the reference's order (default: it is what
    // the log lines are compared on); 1 = sums formed on the device (k_cv_reduce), nothing of size n x D leaves it
    int cv_device = 0;
    DevBuf<double> cv_partial;
    DevBuf<double> es_acc;  // mlggd_error_stats: [4 + MLGGD_MAX_BETAS][D] sums of the call, allocated on first use
    DevBuf<double> ess_acc;  // mlggd_error_stats_signed: [2 MLGGD_MAX_BETAS][D] sums of the call, allocated on first use
    DevBuf<double> os_acc;  // mlggd_output_stats: [4][D] sums of the call, allocated on first use
    // mlggd_set_gv: one equalisation factor per output bin (gv_rule.h).  gv_dev [D] exists from the first set on and is
    // only read by the decoders while gv_on; gv_host [D] is what mlggd_get_gv returns.
    bool gv_on = false;
    DevBuf<float> gv_dev;
    std::vector<float> gv_host;
    int chunk_frames = 0;
    float *in_bunch = nullptr;
    float *in_bunch_buf[2] = {nullptr, nullptr};  // in_bunch alternates between them when bunches are staged ahead
    // noise-aware training (nat_rule.h): nat_frames = cfg.nat_frames > 0 makes layer 0 one stream row wider; nat is the
    // noise table of the CURRENT indexed chunk: the current raw set's own, or the decoder's table of the whole batch
    int nat_frames = 0;
    const float *nat = nullptr;
    // indexed chunk: raw frame streams + first frame of every sample row.  Frame-stream chunks ping-pong
    // between two device buffer sets: the next chunk is uploaded on copy_stream while the kernels of the current one,
    // raw[raw_cur], are still running.  The sizes are those of devbuf_rule.h (feat and nat count FLOATS).
    struct RawSet {
        DevBuf<float> feat, targ;
        DevBuf<int> first;
        // a NAT engine (nat_rule.h): the noise table [n_nat rows][fdim] and the noise row of every sample
        DevBuf<float> nat;
        DevBuf<int> nat_row;
        hipEvent_t last_use = nullptr;  // recorded on the main stream after the last kernel that reads the set
    } raw[2];
    int raw_cur = 0;
    hipStream_t copy_stream = nullptr;
    // mlggd_enhance_waves: device workspace that only grows (ws_grow) and the host copies of the tables and norm
    // vectors it holds, so a call in the steady state allocates nothing and uploads the wave alone
    typedef DevBuf<char> WsBuf;  // bytes: a call takes it as whatever type it needs
    struct WavesWs {
        WsBuf wave, lps, X, blk, out_i, out_f, lps_den, norm, frame_off, out_off, wave_off, utt_of;
        WsBuf nat;  // a NAT engine: the noise rows [n_utts][D] of the batch being decoded
        WsBuf clean, Xc, fstat, sframes, scores;  // mlggd_enhance_waves_scored (score.hip.h)
        WsBuf stoi_utt, stoi_x, stoi_f, stoi_i, stoi_res;  // mlggd_enhance_waves_scored_stoi (stoi.hip.h)
        std::vector<int32_t> h_frame_off, h_utt_of;
        std::vector<long long> h_out_off, h_wave_off;
        std::vector<float> h_norm;  // [2 D]: mean, inv_std as uploaded last
        std::vector<float> h_scores;  // [2 n_utts]: segsnr, lsd as downloaded
        std::vector<StoiUtt> h_stoi_utt;  // [n_utts] as uploaded
        std::vector<float> h_stoi;        // [2 n_utts]: stoi, then the segment counts (int) as downloaded
        int lookup_table = 0;       // utterance of a frame: 0 = binary search over frame_off (default), 1 = per-frame
                                    // table (MLGGD_WAVES_LOOKUP=table, for A/B runs)
    } ww;
    // mlggd_load_waves / mlggd_train_waves (mix.hip.h): the tables of a batch, the mixer's per-utterance words and the
    // noise bank of mlggd_set_noise; the waves and the two LPS streams share ww.wave / ww.clean / ww.lps / ww.lps_den,
    // which every decoding call rewrites from scratch
    struct TrainWs {
        WsBuf norm, frame_off, wave_off, blocks, utt, noise;
        long long n_noise = 0;
        std::vector<float> h_norm;
        std::vector<int32_t> h_frame_off, h_nat_row;
        std::vector<long long> h_wave_off;
        std::vector<mix_rule::Block> h_blocks;
        std::vector<double> h_r;
    } tw;
    int live_groups = 0;  // open live groups (mlggd_live_open): mlggd_destroy refuses while there is one
    bool indexed = false;
    int fdim = 0, toff = 0, raw_frames = 0;
    unsigned step_counter = 0;
    // launch-plan knobs (defaults chosen from measurements; env overrides for A/B runs)
    // 64 x 64-tile forward / dX kernels (kernels64.hip.h): 1 = where the shape gives every CU such a tile (units and
    // frames multiples of 64, tiles >= CUs), 0 = never, 2 = wherever the shape divides (tests, A/B); MLGGD_TILE64
    int tile64 = 1, n_cus = 256;
    int dw_tile = 1, dw_persist = 1, dwp_per_cu = 2, dw_merge = 1, loss_fuse = 1, tile_map = 0, stage_ahead = 1;  // dw_tile 0 = auto

    // data parallel
    int world = 1, rank = 0;
    // data-parallel exchange: 0 = all-reduce of the weight gradients, 1 = all-gather of their FACTORS (the
    // activations Y_{l-1} and dEdX_l of every rank; each rank then forms the global-minibatch gradient itself)
    int dp_mode = 0;  // 2 = gather + SHARDED update: each rank updates its block of weight rows, then W is all-gathered
    int shard_rows[MLGGD_MAXLAYER] = {0};  // 64-row tile rows of layer l owned by each rank
    // Sharded update with the ACTIVATIONS exchanged by all-to-all (MLGGD_DP_MODE=shard_a2a; dp_mode stays 2): rank o
    // forms the gradient of ITS block of weight rows of every layer, for which it needs every rank's Y_{l-1} only in
    // the units of that block -- 1/world of what the all-gather of the whole Y_{l-1} delivers.  The producers write Y
    // (and the staged input rows) blocked by owner (kernels.hip.h y_blocked_base), each block is one message, and
    // what arrives is a plain [world x frames][block width] matrix.  dEdX_l is still all-gathered (every rank needs
    // all of its units).  Per rank and step at 8 x 128 frames, 2827-2048^3-257: 4 + 23 MB of factors + 51 MB of W
    // blocks = 78 MB instead of 106 -- the one built exchange whose link arithmetic fits the >= 6x target.
    int dp_a2a = 0;
    std::vector<float *> Ysrc[MLGGD_MAXLAYER];  // emulated world only: source rank s's blocked Y_l (all owners' blocks)
    hipEvent_t ev_W[MLGGD_MAXLAYER] = {0}, ev_dw_done = nullptr;
    bool ev_W_pending[MLGGD_MAXLAYER] = {false};
    bool fake_world = false;  // test hook: `world` ranks emulated one after the other on this GPU, no communicator
    float *Yall[MLGGD_MAXLAYER] = {0}, *dEdXall[MLGGD_MAXLAYER] = {0};
    // test hook (mlggd_debug_keep_ranks): what emulated ranks 0..world-2 computed in the last step, copied where they
    // produced it (fake_world_prepass) -- the staged input rows, Y_l, dEdX_l and the output, in the engine's layouts
    bool keep_ranks = false;
    std::vector<float *> snap_x, snap_out, snap_y[MLGGD_MAXLAYER], snap_dedx[MLGGD_MAXLAYER];
    hipEvent_t ev_ready = nullptr, ev_gathered = nullptr;
    // fine-grained factor exchange (few ranks: cheap collectives, few links): every factor is sent as soon as it
    // exists, and ev_layer[l] marks the moment both factors of layer l have arrived
    int dp_fine = 1;
    hipEvent_t ev_layer[MLGGD_MAXLAYER] = {0};
    // Collectives that sit ON the step's critical path (the last factor dEdX_1 in front of the dW launch; W_1 in front
    // of the next forward pass) are issued on the MAIN stream: a hop to the communication stream and back costs two
    // event hand-offs of 6-10 us each plus ~5 us of queue bubble per record / wait (1-rank rehearsal, round 3:
    // 30 us between dX_2 and k_dwp, 21 us between k_dwp and the next forward_1).  MLGGD_DP_MAINLINE=0: everything on
    // the communication stream, as in round 2 (A/B).
    int dp_mainline = 1;
    bool comm_after_dw = false;  // the communication stream has already waited on an event recorded after the last dW launch
    RcclComm comm = nullptr;
    // MLGGD_DP_STAT_COMM=1: the 257-float all-reduce of the ML statistic gets a communicator of its own (ncclCommSplit
    // of `comm`), so that it does not queue behind the factor / weight collectives of `comm` that are still in flight
    // (collectives of ONE communicator execute in issue order whatever stream they are on).  Off by default: untested
    // between two GPUs.
    RcclComm stat_comm = nullptr;
    // all-reduce exchange (dp_mode 0): 1 = reduce-scatter of G_l over weight-row blocks, update of this rank's block
    // only, all-gather of the W blocks (same link bytes as the all-reduce, 1/world of the update traffic);
    // 0 (MLGGD_DP_AR_SHARD=0) = all-reduce of G_l and the full update on every rank (rounds 1-3, A/B)
    int ar_shard = 1;
    hipEvent_t ev_grad[MLGGD_MAXLAYER] = {0}, ev_red[MLGGD_MAXLAYER] = {0}, ev_bias = nullptr, ev_bias_red = nullptr;

    // timing
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
    int last_steps = 0;
    bool timing_valid = false;
    // per-kernel-class profiling
    int prof_class = -1, prof_layer = 0, prof_stride = 1;
    std::vector<hipEvent_t> prof_ev;
    size_t prof_used = 0, prof_cap = 0;  // prof_cap = 2 * max_launches of the last select (the pool itself only grows)
    hipEvent_t *prof_attach = nullptr;  // event pair waiting to be attached to the next dW launch
    bool prof_attached = false;
    // Data parallel: an event the communication stream is going to wait for can ride on the producing kernel's own
    // dispatch packet (hipExtLaunchKernelGGL stop event = the packet's completion signal) instead of being a packet of
    // its own behind it: a hipEventRecord on the main queue is a ~5 us bubble between two kernels (round 3, 1-rank
    // rehearsal).  stop_ev_next: attach this event to the next GEMM launch; stop_ev_attached: it was.
    hipEvent_t stop_ev_next = nullptr;
    bool stop_ev_attached = false;
    int dp_stopev = 1;  // MLGGD_DP_STOPEV=0: explicit records (A/B)
    double prof_flops = 0, prof_bytes = 0;

    // diagnostic in-kernel phase stamps (one launch of one (class, layer))
    int stamp_class = -1, stamp_layer = 0, stamp_blocks = 0;
    DevBuf<long long> stamp_buf;  // 8 stamps for each of 8192 blocks, allocated by the first select

    struct DwpTable {  // one cached launch plan of the persistent dW kernel (dwp_table)
        DwpJobs key;
        bool fused;
        int grid;
        DevBuf<DwpDesc> dev;
    };
    std::vector<DwpTable> dwp_tables;
    std::vector<void *> allocs;
    std::vector<const void *> lds_attr_done;  // kernels whose dynamic-LDS limit has been raised on this device

    // a mask engine (mlggd_config.mask_bins = M >= 1, mask_rule.h): D = 2 M outputs, LPS half first.  The scale is read
    // where targets are formed from waves and where a decoder post-filters; mode and thresholds by the decoders alone.
    int mask_bins = 0;
    int mask_mode = mask_rule::kSelect;
    float mask_lo = mask_rule::kLo, mask_hi = mask_rule::kHi, mask_scale = mask_rule::kScale;
    int rbm_open = 0;  // open pre-training sessions (mlggd_rbm_open, at most one): mlggd_destroy refuses while there is one
};

// buffer for the selected launch, nullptr otherwise; one-shot
static long long *stamps_for(mlggd_engine *e, int cls, int layer, int blocks) {
    if (e->stamp_class != cls || e->stamp_layer != layer || !e->stamp_buf.p) return nullptr;
    if ((size_t)blocks * 8 > e->stamp_buf.cap) return nullptr;
    e->stamp_class = -1;
    e->stamp_blocks = blocks;
    return e->stamp_buf.p;
}

// device buffers of one call, freed on every return path
struct DevBufs {
    std::vector<void *> p;
    ~DevBufs() {
        for (void *q : p) hipFree(q);
    }
    template <typename T>
    int alloc(T **out, size_t count) {
        void *q = nullptr;
        HIPCHK(hipMalloc(&q, (count ? count : 1) * sizeof(T)));
        p.push_back(q);
        *out = (T *)q;
        return MLGGD_OK;
    }
    // ... and filled from host memory by a blocking copy on the null stream (the one-shot device entries)
    template <typename T>
    int upload(T **out, const T *host, size_t count) {
        CHK(alloc(out, count));
        if (count) HIPCHK(hipMemcpy(*out, host, count * sizeof(T), hipMemcpyHostToDevice));
        return MLGGD_OK;
    }
};

static int dev_alloc(mlggd_engine *e, float **p, size_t count) {
    // +64 floats of slack; zero-filled like the reference's devnew_vf (BP_GPU.cu:528-543)
    const size_t bytes = (count + 64) * sizeof(float);
    HIPCHK(hipMalloc((void **)p, bytes));
    // on the engine's own (non-blocking) stream: a null-stream memset would not be ordered
    // before later uploads on e->stream
    HIPCHK(hipMemsetAsync(*p, 0, bytes, e->stream));
    e->allocs.push_back(*p);
    return MLGGD_OK;
}

static int upload_padded(float *dst, int Np, const float *src, int K, int N, hipStream_t st) {
    // [K][N] compact -> [Kp][Np] padded rows
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)Np * 4, src, (size_t)N * 4, (size_t)N * 4, K, hipMemcpyHostToDevice, st));
    return MLGGD_OK;
}
static int download_padded(float *dst, const float *src, int Np, int K, int N, hipStream_t st) {
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)N * 4, src, (size_t)Np * 4, (size_t)N * 4, K, hipMemcpyDeviceToHost, st));
    return MLGGD_OK;
}

// ------------------------------------------------------------------ kernel launch plan
// Times the launches of one kernel class with a pair of HIP events per launch (mlggd_profile_select).
// The GEMM kernels (classes "dw", "fwd", "dx") take the pair INTO the launch (hipExtLaunchKernelGGL start / stop
// events = the dispatch's own begin / end timestamps, what rocprofv3 reports as the kernel's duration); the other
// classes are bracketed by events recorded on the stream before and after, which adds the cost of the bracket.
struct ProfScope {
    mlggd_engine *e;
    bool on, attach;
    ProfScope(mlggd_engine *eng, int cls, int layer)
        : e(eng), on(false), attach(cls == KC_DW || cls == KC_FWD || cls == KC_DX) {
        if (e->prof_class == cls && (e->prof_layer == 0 || e->prof_layer == layer) &&
            e->step_counter % (unsigned)e->prof_stride == 0 && e->prof_used + 2 <= e->prof_cap) {
            on = true;
            if (attach) {
                e->prof_attach = &e->prof_ev[e->prof_used];  // consumed by the launch itself
                e->prof_attached = false;
            } else if (hipEventRecord(e->prof_ev[e->prof_used], e->stream) != hipSuccess) {
                on = false;
            }
        }
    }
    ~ProfScope() {
        if (!on) return;
        if (attach) {
            e->prof_attach = nullptr;
            if (e->prof_attached) e->prof_used += 2;
        } else if (hipEventRecord(e->prof_ev[e->prof_used + 1], e->stream) == hipSuccess) {
            e->prof_used += 2;
        }
    }
};
// launch a GEMM kernel, with the pending event pair of the profiler attached if there is one
template <typename F, typename... Args>
static void launch_timed(mlggd_engine *e, F kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    if (e->prof_attach && !e->prof_attached) {
        hipExtLaunchKernelGGL(kernel, grid, block, (std::uint32_t)lds, st, e->prof_attach[0], e->prof_attach[1], 0u, args...);
        e->prof_attached = true;
    } else if (e->stop_ev_next && !e->stop_ev_attached) {
        hipExtLaunchKernelGGL(kernel, grid, block, (std::uint32_t)lds, st, (hipEvent_t) nullptr, e->stop_ev_next, 0u, args...);
        e->stop_ev_attached = true;
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    }
}

static int launch_check(const char *what) {
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(MLGGD_ERR_DEVICE, "launch of %s failed: %s", what, hipGetErrorString(err));
    return MLGGD_OK;
}

template <typename F>
static int ensure_lds(mlggd_engine *e, F fn, size_t bytes) {
    // kernels with > 64 KB of dynamic LDS need the attribute.  It is a per-device property of the loaded code
    // object, so the "already set" list lives in the engine (one engine = one device), not in the process.
    const void *key = (const void *)fn;
    for (const void *d : e->lds_attr_done)
        if (d == key) return MLGGD_OK;
    HIPCHK(hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    e->lds_attr_done.push_back(key);
    return MLGGD_OK;
}

static int log2_or_minus1(int d) {  // for divmod_by in the kernels
    for (int sft = 0; sft < 31; sft++)
        if (d == (1 << sft)) return sft;
    return -1;
}
static FwdArgs fwd_args(mlggd_engine *e, int l, float *Yrow_out) {
    FwdArgs a{};
    a.W = e->W[l];
    a.Yt_in = e->Yt[l - 1];
    a.bias = e->bias[l];
    a.Yt_out = e->Yt[l];
    a.Y_out = Yrow_out;
    a.slab = e->slab;
    a.Kp = e->lsp[l - 1];
    a.Np = e->lsp[l];
    a.Bp = e->Bp;
    a.N = e->ls[l];
    a.n_tiles = e->lsp[l] / 32;
    a.b_tiles = e->Bp / 32;
    a.S = (l == e->L - 1) ? e->S_out : 1;
    a.map = e->tile_map;
    a.b_shift = log2_or_minus1(a.b_tiles);
    a.s_shift = log2_or_minus1(a.S);
    a.yblk = (e->dp_a2a && l < e->L - 1) ? e->shard_rows[l + 1] * 64 : 0;  // Y_l is layer l+1's K-side factor
    return a;
}

static DxArgs dx_args(mlggd_engine *e, int l) {
    DxArgs a{};
    a.W = e->W[l];
    a.dEdXt = e->dEdXt[l];
    a.Yt_prev = e->Yt[l - 1];
    a.dEdXt_prev = e->dEdXt[l - 1];
    a.dEdX_prev = e->dEdX[l - 1];
    a.Kp = e->lsp[l - 1];
    a.Np = e->lsp[l];
    a.Bp = e->Bp;
    a.k_tiles = e->lsp[l - 1] / 32;
    a.b_tiles = e->Bp / 32;
    a.map = e->tile_map;
    a.b_shift = log2_or_minus1(a.b_tiles);
    return a;
}

static DwpArgs dwp_args(mlggd_engine *e, int l, const float *in_rows, const float *Yrow_prev) {
    DwpArgs a;
    memset(&a, 0, sizeof(a));
    const int Kp = e->lsp[l - 1], Np = e->lsp[l];
    a.Yrow = (l == 1) ? in_rows : Yrow_prev;
    a.dEdX = e->dEdX[l];
    a.Wt = e->W[l];
    a.delta = e->dW[l];
    a.G = e->G[l];
    a.bias = e->bias[l];
    a.dbias = e->dbias[l];
    a.gb = e->gb[l];
    a.ldA = Kp;  // layer 1 reads the staged, padded copy of the minibatch's rows (in_bunch), not the caller's chunk
    a.K = e->ls[l - 1];
    a.N = e->ls[l];
    a.Kp = Kp;
    a.Np = Np;
    a.n_wg = (Np + 63) / 64;
    a.ntiles = ((Kp + 63) / 64) * a.n_wg;
    a.k_first = 0;
    a.wd_off = 0;
    a.do_bias = 1;
    return a;
}
// what every tile of a launch shares.  frames: rows of the minibatch the jobs' operands hold (e->B on one device,
// world * Bp over gathered factors)
static DwpConst dwp_const(const mlggd_engine *e, float nf, int frames) {
    DwpConst C;
    C.B = frames;
    C.nf = nf;
    C.mom = e->cfg.momentum;
    C.lr = e->cfg.lrate;
    C.wc = e->cfg.weightcost;
    return C;
}

// one minibatch of the resident chunk: expanded rows, or raw streams + per-row first frame
struct Bunch {
    const float *in;    // expanded: first row of the bunch; indexed: the raw feature stream
    const float *targ;  // expanded: first target row;       indexed: the raw target stream
    const int *first;   // indexed: first frame of each sample row of this bunch, else nullptr
    const int *nat_row; // indexed chunk of a NAT engine: the noise row of each sample row of this bunch, else nullptr
};
static Bunch bunch_at(mlggd_engine *e, int sample) {
    Bunch b;
    if (e->indexed) {
        const mlggd_engine::RawSet &r = e->raw[e->raw_cur];
        b.in = r.feat.p;
        b.targ = r.targ.p;
        b.first = r.first.p + sample;
        b.nat_row = e->nat_frames ? r.nat_row.p + sample : nullptr;
    } else {
        b.in = e->chunk_in.p + (size_t)sample * e->K0;
        b.targ = e->chunk_targ.p + (size_t)sample * e->D;
        b.first = nullptr;
        b.nat_row = nullptr;
    }
    return b;
}
// row-major [Bp][lsp[0]] copy of the bunch (16-byte aligned rows, zero pads) written by the input-staging kernel:
// the layer-1 dW operand, the data-parallel input factor and what dropout masks
static const float *bunch_rows(mlggd_engine *e, const Bunch &) { return e->in_bunch; }

static StageArgs stage_args(mlggd_engine *e, const Bunch &bn, int frames, float *rows_out) {
    StageArgs a;
    a.in = bn.in;
    a.ld = e->K0;
    a.B = frames;
    a.K = e->K0;
    a.Kp = e->lsp[0];
    a.inT = e->Yt[0];
    a.Bp = e->Bp;
    a.b_tiles = e->Bp / 32;
    a.first = bn.first;
    a.fdim = e->fdim;
    a.rows_out = rows_out;
    a.yblk = e->dp_a2a ? e->shard_rows[1] * 64 : 0;  // the staged rows are layer 1's K-side factor
    return a;
}
static int stage_blocks(const mlggd_engine *e) { return (e->lsp[0] / 32) * (e->Bp / 32); }
// the other half of the in_bunch double buffer (target of a bunch staged one step ahead)
static float *in_bunch_other(mlggd_engine *e) {
    return e->in_bunch == e->in_bunch_buf[0] ? e->in_bunch_buf[1] : e->in_bunch_buf[0];
}

// Which GEMM form a layer takes.  fwd: layer l's forward (output tile over units of l x frames); dx: the dX launched for
// layer l (output tile over units of l-1 x frames).  The 64 x 64 form needs a whole number of such tiles and -- unless
// forced -- at least one per CU; the output layer always takes the slab form (small N: K split over workgroups).
static bool tile64_ok(const mlggd_engine *e, int units_p) {
    if (e->tile64 == 0 || units_p % 64 != 0 || e->Bp % 64 != 0) return false;
    return e->tile64 == 2 || (long)(units_p / 64) * (e->Bp / 64) >= e->n_cus;
}
static bool fwd64_used(const mlggd_engine *e, int l) {
    if (!tile64_ok(e, e->lsp[l])) return false;
    return l != e->L - 1 || e->S_out == 1;  // an output layer only when it needs no split-K slabs (it is that wide)
}
static bool dx64_used(const mlggd_engine *e, int l) {
    return l >= 2 && tile64_ok(e, e->lsp[l - 1]);
}
// Which of k_dx's two forms a launch over Kp units takes.  Both are 4 waves with the main loop software-pipelined inside
// the wave.  Operands by LDS-DMA (136 KB of LDS) where one workgroup per CU is all there is: <= 256 workgroups.  Through
// staging registers (71 KB: two workgroups per CU) above that.  run_dx and the RBM's down-pass (rbm.hip.h) both ask here.
static bool dx_dma(const mlggd_engine *e, int Kp) { return (Kp / 32) * (e->Bp / 32) <= 256; }

static int run_transpose(mlggd_engine *e, const Bunch &bn, int frames) {
    ProfScope ps(e, KC_TRANSPOSE, 0);
    if (bn.nat_row) {  // a NAT engine's frame stream: the window, then the noise row of the sample's utterance
        hipLaunchKernelGGL(k_transpose_in_nat, dim3(stage_blocks(e)), dim3(256), 0, e->stream,
                           stage_args(e, bn, frames, e->in_bunch), e->nat, bn.nat_row);
        return launch_check("k_transpose_in_nat");
    }
    hipLaunchKernelGGL(k_transpose_in, dim3(stage_blocks(e)), dim3(256), 0, e->stream,
                       stage_args(e, bn, frames, e->in_bunch));
    return launch_check("k_transpose_in");
}

// every consumer of W on the main stream first waits for the all-gathers of the previous step
static int wait_weight_gathers(mlggd_engine *e, int l_lo, int l_hi) {
    for (int l = l_lo; l <= l_hi; l++)
        if (e->ev_W_pending[l]) {
            HIPCHK(hipStreamWaitEvent(e->stream, e->ev_W[l], 0));
            e->ev_W_pending[l] = false;
        }
    return MLGGD_OK;
}

static int run_dropout(mlggd_engine *e, int layer, const float *chunk_rows) {
    // BP_GPU.cu:344-355: visible_omit on the input, hid_omit on hidden activations
    const float p = (layer == 0) ? e->cfg.visible_omit : e->cfg.hid_omit;
    const size_t n = (size_t)e->lsp[layer] * e->Bp;
    float *rows = (layer == 0) ? const_cast<float *>(chunk_rows) : e->Y[layer];
    const int ld = e->lsp[layer];
    hipLaunchKernelGGL(k_dropout, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, e->Yt[layer], rows,
                       e->ls[layer], e->lsp[layer], ld, e->B, e->Bp, p, (unsigned)e->cfg.random_seed,
                       e->step_counter * 16u + (unsigned)layer);
    return launch_check("k_dropout");
}

// prestaged: Yt[0] (and, for frame-stream chunks, the other in_bunch buffer) already hold this
// bunch -- the previous training step staged it alongside its loss kernel
static int gather_begin(mlggd_engine *e, bool already_ordered);
static int gather_end(mlggd_engine *e);
static void gather_arm(mlggd_engine *e);
static int gather_begin_armed(mlggd_engine *e);
static int gather_one(mlggd_engine *e, const float *src, float *dst, size_t count, hipStream_t st);
static int exchange_y(mlggd_engine *e, int l, const float *src, hipStream_t st);
enum { GATHER_INPUT = 1, GATHER_HIDDEN = 2, GATHER_HIDDEN_EACH = 4 };  // data-parallel factor exchange issued from inside the forward pass

// A hidden layer's 32 x 32-tile forward launch.  k_fwd has one form: 4 waves, the main loop software-pipelined inside the
// wave, operands by LDS-DMA.  The stamped instantiation only when this launch was picked for stamps (kernels.hip.h k_fwd).
template <int MODE>
static int launch_fwd(mlggd_engine *e, int nwg, const FwdArgs &fa, long long *st) {
    const size_t lds = fwd_lds_floats<4, 4>() * sizeof(float);
    if (st) {
        CHK(ensure_lds(e, k_fwd<MODE, 4, 4, true>, lds));
        launch_timed(e, k_fwd<MODE, 4, 4, true>, dim3(nwg), dim3(256), lds, e->stream, fa, st);
    } else {
        CHK(ensure_lds(e, k_fwd<MODE, 4, 4, false>, lds));
        launch_timed(e, k_fwd<MODE, 4, 4, false>, dim3(nwg), dim3(256), lds, e->stream, fa, st);
    }
    return MLGGD_OK;
}

static int run_forward(mlggd_engine *e, const Bunch &bn, int frames, bool training, bool prestaged = false,
                       int gather_flags = 0, int l_end = 0) {  // l_end > 0: layers 1 .. l_end - 1 only (rbm.hip.h)
    e->stop_ev_next = nullptr;  // an event armed by a launch sequence that bailed out early must not ride on an unrelated launch
    e->stop_ev_attached = false;
    if (prestaged) {
        e->in_bunch = in_bunch_other(e);
    } else {
        CHK(run_transpose(e, bn, frames));
    }
    const float *in_rows = bunch_rows(e, bn);
    if (gather_flags & GATHER_INPUT) {  // the input rows can travel from the first microsecond of the step
        // prestaged rows were written by the previous step's loss launch and Yall[0] was last read by its dW launch: if
        // the communication stream has already waited on an event recorded after that launch (sharded update: the W
        // gathers did), it needs no new event
        CHK(gather_begin(e, prestaged && e->comm_after_dw && e->dp_mainline));
        CHK(exchange_y(e, 0, in_rows, nullptr));
        CHK(gather_end(e));
    }
    e->comm_after_dw = false;
    const int b_tiles = e->Bp / 32;
    const bool drop = training && e->cfg.dropoutflag == 1;
    const bool cvscale = !training && e->cfg.dropoutflag == 1;
    const bool relu = e->cfg.activation == MLGGD_ACT_RELU;  // the hidden layers' epilogue: a host-side choice of instantiation
    if (drop) CHK(run_dropout(e, 0, in_rows));
    for (int l = 1; l < (l_end > 0 ? l_end : e->L); l++) {
        const int Kp = e->lsp[l - 1], Np = e->lsp[l], n_tiles = Np / 32;
        CHK(wait_weight_gathers(e, l, l));  // sharded data parallel: W_l of the previous step may still be arriving
        if (cvscale) {  // DevWeightMultiP before the GEMM, BP_GPU.cu:484-489
            const float keep = 1.0f - ((l == 1) ? e->cfg.visible_omit : e->cfg.hid_omit);
            hipLaunchKernelGGL(k_scale, dim3(1024), dim3(256), 0, e->stream, e->W[l], (size_t)Kp * Np, keep);
        }
        {
            // this layer's activations are sent right after the launch: the event rides on it
            if (((gather_flags & GATHER_HIDDEN_EACH) && l < e->L - 1) || ((gather_flags & GATHER_HIDDEN) && l == e->L - 2))
                gather_arm(e);
            ProfScope ps(e, KC_FWD, l);
            FwdArgs fa = fwd_args(e, l, e->Y[l]);
            if (fwd64_used(e, l)) {
                fa.n_tiles = Np / 64;
                fa.b_tiles = e->Bp / 64;
                fa.b_shift = log2_or_minus1(fa.b_tiles);
                const size_t lds = t64_lds_floats() * sizeof(float);
                if (l != e->L - 1 && relu) {
                    CHK(ensure_lds(e, k_fwd64<FWD_RELU>, lds));
                    launch_timed(e, k_fwd64<FWD_RELU>, dim3(fa.n_tiles * fa.b_tiles), dim3(256), lds, e->stream, fa);
                } else if (l != e->L - 1) {
                    CHK(ensure_lds(e, k_fwd64<FWD_SIGMOID>, lds));
                    launch_timed(e, k_fwd64<FWD_SIGMOID>, dim3(fa.n_tiles * fa.b_tiles), dim3(256), lds, e->stream, fa);
                } else {
                    CHK(ensure_lds(e, k_fwd64<FWD_SLAB>, lds));
                    launch_timed(e, k_fwd64<FWD_SLAB>, dim3(fa.n_tiles * fa.b_tiles), dim3(256), lds, e->stream, fa);
                }
            } else if (l != e->L - 1) {
                long long *st = stamps_for(e, KC_FWD, l, n_tiles * b_tiles);
                if (relu) CHK(launch_fwd<FWD_RELU>(e, n_tiles * b_tiles, fa, st));
                else CHK(launch_fwd<FWD_SIGMOID>(e, n_tiles * b_tiles, fa, st));
            } else {
                const int nwg = n_tiles * b_tiles * e->S_out;
                const size_t lds = fwd_lds_floats<4, 4>() * sizeof(float);
                CHK(ensure_lds(e, k_fwd<FWD_SLAB, 4, 4>, lds));
                launch_timed(e, k_fwd<FWD_SLAB, 4, 4>, dim3(nwg), dim3(256), lds, e->stream, fa, (long long *)nullptr);
            }
        }
        CHK(launch_check("k_fwd"));
        if (cvscale) {  // BP_GPU.cu:496-501
            const float keep = 1.0f - ((l == 1) ? e->cfg.visible_omit : e->cfg.hid_omit);
            hipLaunchKernelGGL(k_scale, dim3(1024), dim3(256), 0, e->stream, e->W[l], (size_t)Kp * Np, 1.0f / keep);
        }
        if (drop && l != e->L - 1) CHK(run_dropout(e, l, nullptr));
        if ((gather_flags & GATHER_HIDDEN_EACH) && l < e->L - 1) {  // each hidden layer's activations at once
            CHK(gather_begin_armed(e));
            CHK(exchange_y(e, l, e->Y[l], nullptr));
            CHK(gather_end(e));
        }
        if ((gather_flags & GATHER_HIDDEN) && l == e->L - 2) {  // all hidden activations exist: send them
            CHK(gather_begin_armed(e));                         // beside the output layer, the loss and dX
            for (int g = 1; g < e->L - 1; g++) CHK(exchange_y(e, g, e->Y[g], nullptr));
            CHK(gather_end(e));
        }
    }
    return MLGGD_OK;
}

template <int T>
static int launch_dw(mlggd_engine *e, int l, const float *in_rows, bool fused, float nf) {
    const int Kp = e->lsp[l - 1], Np = e->lsp[l];
    const int k_wg = (Kp + 64 * T - 1) / (64 * T), n_wg = (Np + 64 * T - 1) / (64 * T);
    const float *A = (l == 1) ? in_rows : e->Y[l - 1];
    const int ldA = Kp;
    const size_t lds = (size_t)2 * (64 * T) * (64 * T) * sizeof(float);
    if (fused) CHK(ensure_lds(e, k_dw<T, true>, lds));
    else CHK(ensure_lds(e, k_dw<T, false>, lds));
    if (fused)
        launch_timed(e, k_dw<T, true>, dim3(k_wg * n_wg), dim3(256), lds, e->stream, A, ldA, (const float *)e->dEdX[l], e->W[l],
                     e->dW[l], (float *)nullptr, e->bias[l], e->dbias[l], (float *)nullptr, e->ls[l - 1], e->ls[l], Np,
                     e->B, e->Bp, n_wg, nf, e->cfg.momentum, e->cfg.lrate, e->cfg.weightcost,
                     stamps_for(e, KC_DW, l, k_wg * n_wg));
    else
        launch_timed(e, k_dw<T, false>, dim3(k_wg * n_wg), dim3(256), lds, e->stream, A, ldA, (const float *)e->dEdX[l], e->W[l],
                     e->dW[l], e->G[l], e->bias[l], e->dbias[l], e->gb[l], e->ls[l - 1], e->ls[l], Np, e->B, e->Bp, n_wg,
                     nf, e->cfg.momentum, e->cfg.lrate, e->cfg.weightcost, (long long *)nullptr);
    return launch_check("k_dw");
}

// persistent pipelined dW (+update) kernel: Bp = 64*H
static int dwp_grid(mlggd_engine *e, int ntiles) {
    int grid = 256 * (e->dwp_per_cu > 0 ? e->dwp_per_cu : 2);
    return grid > ntiles ? ntiles : grid;
}
// jobs for layers lhi, lhi-1, ..., llo in one launch
static_assert(DWP_MAXJOBS >= MLGGD_MAXLAYER, "job table too small");
static DwpJobs dwp_jobs(mlggd_engine *e, int lhi, int llo, const float *in_rows) {
    DwpJobs J;
    memset(&J, 0, sizeof(J));
    int nj = 0, end = 0;
    for (int l = lhi; l >= llo; l--) {
        J.job[nj] = dwp_args(e, l, in_rows, e->Y[l - 1]);
        end += J.job[nj].ntiles;
        J.tile_end[nj++] = end;
    }
    J.njobs = nj;
    J.total = end;
    return J;
}
// The per-tile records the persistent dW kernel walks (kernels.hip.h DwpDesc), built once per launch plan and
// kept on the device: the plan is the job list (which layers / row blocks / operands) and the grid.  A training
// run uses two plans (the layer-1 operand alternates between the two staged-row buffers), a data-parallel run
// a few more.  Hyper-parameters and the frame count are not part of the plan: they travel in DwpConst with every launch.
// The cache is keyed on the job list with memcmp: a value comparison as long as this holds (every builder starts from
// zeroed storage, so the unused job slots are equal too).
static_assert(std::has_unique_object_representations_v<DwpJobs>, "padding or a float in DwpJobs: memcmp is no comparison");
static int dwp_table(mlggd_engine *e, const DwpJobs &J, bool fused, int grid, const DwpDesc **out) {
    for (const auto &t : e->dwp_tables)
        if (t.fused == fused && t.grid == grid && memcmp(&t.key, &J, sizeof(J)) == 0) {
            *out = t.dev.p;
            return MLGGD_OK;
        }
    // A run uses two plans on one GPU (the layer-1 operand alternates between the two staged-row buffers) and a
    // handful more in the data-parallel modes.  A miss costs a hipMalloc and a blocking copy in the middle of a
    // step, so a plan count that keeps growing is a bug (a key that never matches): fail loudly, do not leak.
    if (e->dwp_tables.size() >= 64)
        return fail(MLGGD_ERR_STATE, "dW tile table: %zu launch plans cached and still missing -- plan key unstable",
                    e->dwp_tables.size());
    std::vector<DwpDesc> recs((size_t)J.total + 2 * (size_t)grid);
    size_t n = 0;
    for (int j = 0; j < J.njobs; j++) {
        const DwpArgs &a = J.job[j];
        // the kernel's out-of-range vector offset + 24 rows must stay below 2^31 (kernels.hip.h DWP_OFF0)
        if (a.Np >= (1 << 17)) return fail(MLGGD_ERR_ARG, "dW tile table: layer of %d units is too wide", a.Np);
        for (int tl = 0; tl < a.ntiles; tl++, n++) {
            const int kt = a.k_first + tl / a.n_wg, nt = tl % a.n_wg;
            const int k0 = kt * 64, n0 = nt * 64;
            DwpDesc &d = recs[n];
            d.A = a.Yrow + (k0 - a.k_base);
            d.Bm = a.dEdX + n0;
            const size_t base = (size_t)k0 * a.Np + n0;
            int rows = a.K - k0;
            rows = rows < 0 ? 0 : rows > 64 ? 64 : rows;
            if (a.wd_off) {  // bias-only tile: W / delta are neither read nor written
                rows = 0;
                d.W = a.Wt;
                d.D = a.delta;
                d.szW = 0;
            } else {
                d.W = (fused ? a.Wt : a.G) + base;
                d.D = fused ? a.delta + base : nullptr;
                // the stores may touch the tile's real rows and nothing behind them: rows >= `rows` lie beyond
                // num_records, so the range check is the row test (pad rows are never written)
                const size_t to_end = ((size_t)a.Kp * a.Np - base) * sizeof(float);
                const size_t to_row = (size_t)rows * a.Np * sizeof(float);
                d.szW = (unsigned)(to_end < to_row ? to_end : to_row);
            }
            const int colsw = a.Np - n0 < 64 ? a.Np - n0 : 64;
            int nbias = (a.do_bias && kt == 0) ? a.N - n0 : 0;
            nbias = nbias < 0 ? 0 : nbias > 64 ? 64 : nbias;
            d.bias = (fused ? a.bias : a.gb) + n0;
            d.dbias = fused ? a.dbias + n0 : nullptr;
            d.ldA = a.ldA;
            d.Np = a.Np;
            d.packed = (unsigned)rows | ((unsigned)colsw << 8) | ((unsigned)nbias << 16) | (1u << 24);
        }
    }
    if (n != (size_t)J.total) return fail(MLGGD_ERR_STATE, "dW tile table: %zu records for %d tiles", n, J.total);
    for (; n < recs.size(); n++) {  // "no such tile": empty descriptors -- loads return zeros, stores are dropped
        DwpDesc &d = recs[n];
        d = recs[0];
        d.packed = 0;
        d.szW = 0;
    }
    mlggd_engine::DwpTable t;
    t.key = J;
    t.fused = fused;
    t.grid = grid;
    HIPCHK(t.dev.grow(recs.size(), recs.size(), e->bufs, nullptr, nullptr));
    // pageable source, synchronous copy: complete when the call returns, so the launch that follows sees it
    HIPCHK(hipMemcpy(t.dev.p, recs.data(), recs.size() * sizeof(DwpDesc), hipMemcpyHostToDevice));
    *out = t.dev.p;
    e->dwp_tables.push_back(std::move(t));
    return MLGGD_OK;
}

// G / n is a multiply when n, the frame count as the kernels get it, is a power of two >= 1 (bit-identical, see
// kernels.hip.h POW2)
static bool pow2_frames(float nf) {
    unsigned bits;
    memcpy(&bits, &nf, sizeof(bits));
    return (bits & 0x007FFFFFu) == 0u && nf >= 1.0f;
}
// one launch of k_dwp<H, FUSED, POW2>: the stamped instantiation only when the launch was picked for stamps
// (kernels.hip.h k_fwd).  bias_only (FUSED plans only): k_dwp_bias<H, POW2> in its place, by a plain launch -- the
// profiler's event pair and an armed stop event belong to the launch of the weight tiles that follows it.
template <int H, bool FUSED, bool POW2>
static int launch_dwp_k(mlggd_engine *e, int grid, const DwpDesc *table, int total, const DwpConst &C, bool bias_only,
                        long long *stamps) {
    const size_t lds = dwp_lds_floats() * sizeof(float);
    if constexpr (FUSED) {
        if (bias_only) {
            CHK(ensure_lds(e, k_dwp_bias<H, POW2>, lds));
            hipLaunchKernelGGL((k_dwp_bias<H, POW2>), dim3(grid), dim3(256), lds, e->stream, table, total, C, (long long *)nullptr);
            return launch_check("k_dwp_bias");
        }
    }
    if (stamps) {
        CHK(ensure_lds(e, k_dwp<H, FUSED, POW2, true>, lds));
        launch_timed(e, k_dwp<H, FUSED, POW2, true>, dim3(grid), dim3(256), lds, e->stream, table, total, C, stamps);
    } else {
        CHK(ensure_lds(e, k_dwp<H, FUSED, POW2, false>, lds));
        launch_timed(e, k_dwp<H, FUSED, POW2, false>, dim3(grid), dim3(256), lds, e->stream, table, total, C, stamps);
    }
    return launch_check("k_dwp");
}
template <int H>
static int launch_dwp_t(mlggd_engine *e, const DwpJobs &J, const DwpConst &C, bool fused, int stamp_layer) {
    const int grid = dwp_grid(e, J.total);
    if (J.total < 1) return MLGGD_OK;
    const DwpDesc *table = nullptr;
    bool bias_only = J.njobs > 0, any_bias_only = false;  // only the sharded data-parallel plans hold bias-only jobs
    for (int j = 0; j < J.njobs; j++) {
        bias_only = bias_only && J.job[j].wd_off != 0;
        any_bias_only = any_bias_only || J.job[j].wd_off != 0;
    }
    if (any_bias_only && (!bias_only || !fused))
        return fail(MLGGD_ERR_STATE, "bias-only jobs need a launch of their own on the fused path");
    // (from here on bias_only == any_bias_only)
    CHK(dwp_table(e, J, fused, grid, &table));
    const bool pow2 = pow2_frames(C.nf);
    long long *stamps = nullptr;
    if (!bias_only) {
        if constexpr (H == 2 || H == 8) {
            if (e->stamp_class == KC_DW && e->stamp_layer == -1 && e->stamp_buf.p && fused && C.nf == 128.0f) {
                // diagnostic: the twin kernel with per-phase cycle sums (rows grid .. 2*grid-1 of the stamp buffer)
                long long *sp = stamps_for(e, KC_DW, -1, 2 * grid);
                if (sp) {
                    const size_t lds = dwp_lds_floats() * sizeof(float);
                    CHK(ensure_lds(e, k_dwp_phases<H>, lds));
                    hipLaunchKernelGGL((k_dwp_phases<H>), dim3(grid), dim3(256), lds, e->stream, table, J.total, C, sp);
                    return launch_check("k_dwp_phases");
                }
            }
        }
        stamps = stamps_for(e, KC_DW, stamp_layer, grid);
    }
    if (fused)
        return pow2 ? launch_dwp_k<H, true, true>(e, grid, table, J.total, C, bias_only, stamps)
                    : launch_dwp_k<H, true, false>(e, grid, table, J.total, C, bias_only, stamps);
    return pow2 ? launch_dwp_k<H, false, true>(e, grid, table, J.total, C, false, stamps)
                : launch_dwp_k<H, false, false>(e, grid, table, J.total, C, false, stamps);
}
static bool dwp_usable(const mlggd_engine *e) {
    const int Hh = e->Bp / 64;
    return e->dw_persist && e->Bp % 64 == 0 && (Hh == 1 || Hh == 2 || Hh == 4 || Hh == 8);
}
// units: 64-frame units per tile = (frames the jobs' operands hold) / 64
static int launch_dwp(mlggd_engine *e, const DwpJobs &J, const DwpConst &C, bool fused, int stamp_layer, int units = 0) {
    switch (units > 0 ? units : e->Bp / 64) {
    case 1: return launch_dwp_t<1>(e, J, C, fused, stamp_layer);
    case 2: return launch_dwp_t<2>(e, J, C, fused, stamp_layer);
    case 4: return launch_dwp_t<4>(e, J, C, fused, stamp_layer);
    case 8: return launch_dwp_t<8>(e, J, C, fused, stamp_layer);
    case 16: return launch_dwp_t<16>(e, J, C, fused, stamp_layer);
    default: return fail(MLGGD_ERR_STATE, "no dW kernel for %d units per tile", units);
    }
}

// ---- data-parallel exchange by all-gather of the gradient's factors (dp_mode 1) -------------------
// G_l = sum over ranks of Y_{l-1,r}^T dEdX_{l,r} is a product of [frames x units] matrices that are 8-16 x
// smaller than G_l itself at 128 frames per rank (7.9 MB of factors vs 58.8 MB of gradients per rank and
// step), so the ranks exchange the factors: every rank gathers all ranks' Y_{l-1} and dEdX_l (rank-major
// rows = the rows of ONE minibatch of world*B frames) and runs the same fused dW + update kernel over the
// global minibatch.  All ranks compute bit-identical updates, so no gradient, bias or weight ever crosses
// the links, there is no separate update pass, and the result is exactly the single-device step with
// bunchsize world*B.  The price is world x the dW MFMA work per rank.
static bool gather_usable(const mlggd_engine *e, int world) {
    const long frames = (long)world * e->Bp;
    const long units = frames / 64;
    return e->dw_persist && e->B == e->Bp && frames % 64 == 0 &&
           (units == 1 || units == 2 || units == 4 || units == 8 || units == 16);
}
static int gather_alloc(mlggd_engine *e) {
    const size_t rows = (size_t)e->world * e->Bp;
    for (int l = 0; l < e->L - 1; l++) {
        // all-to-all form: this rank's block of units from every rank ([world x Bp][block width]); shard_alloc ran first
        const size_t width = e->dp_a2a ? (size_t)e->shard_rows[l + 1] * 64 : (size_t)e->lsp[l];
        CHK(dev_alloc(e, &e->Yall[l], rows * width));
        if (e->dp_a2a) {
            // the producers write Y_l (l = 0: the staged rows, two buffers) blocked by owner: world blocks of [Bp][width]
            if (l == 0) {
                CHK(dev_alloc(e, &e->in_bunch_buf[0], rows * width));
                CHK(dev_alloc(e, &e->in_bunch_buf[1], rows * width));
                e->in_bunch = e->in_bunch_buf[0];
            } else {
                CHK(dev_alloc(e, &e->Y[l], rows * width));
            }
            if (e->fake_world)
                for (int s = 0; s + 1 < e->world; s++) {
                    float *q = nullptr;
                    CHK(dev_alloc(e, &q, rows * width));
                    e->Ysrc[l].push_back(q);
                }
        }
    }
    for (int l = 1; l < e->L; l++) CHK(dev_alloc(e, &e->dEdXall[l], rows * e->lsp[l]));
    HIPCHK(hipEventCreateWithFlags(&e->ev_ready, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&e->ev_gathered, hipEventDisableTiming));
    for (int l = 1; l < e->L; l++) HIPCHK(hipEventCreateWithFlags(&e->ev_layer[l], hipEventDisableTiming));
    // Default: the GROUPED factor exchange (four exchanges per step) at every world size.  Round 2 chose the
    // fine-grained form (every factor sent the moment it exists, dW launch split in two) up to 5 ranks on a link model;
    // round 3 measured what it costs before any link time -- +15 us of device time per step (seven more hand-offs
    // between the streams) and twice the host enqueue time (143 vs 70 us per step, next to a 170 us device step) --
    // against a modelled gain of ~20 us of hidden link time at 2 ranks.  MLGGD_DP_FINE=1 selects it; bench.py measures
    // both forms in every multi-GPU run (dp_arms.gather_other_granularity).
    if (const char *v = getenv("MLGGD_DP_FINE")) e->dp_fine = atoi(v);
    else e->dp_fine = 0;
    return MLGGD_OK;
}
// Launch-order knobs of every data-parallel mode (A/B switches; the defaults rest on a 1-rank rehearsal and on
// emulated worlds -- nothing has run between two GPUs yet).
static void dp_knobs(mlggd_engine *e) {
    if (const char *v = getenv("MLGGD_DP_MAINLINE")) e->dp_mainline = atoi(v);
    if (const char *v = getenv("MLGGD_DP_STOPEV")) e->dp_stopev = atoi(v);
    if (const char *v = getenv("MLGGD_DP_AR_SHARD")) e->ar_shard = atoi(v) != 0;
}
// one rank's block -> every rank's slot r of dst (on the communication stream, or on `st`)
static int gather_one(mlggd_engine *e, const float *src, float *dst, size_t count, hipStream_t st = nullptr) {
    if (!st) st = e->comm_stream;
    if (e->fake_world) {  // the other ranks' slots were filled by fake_world_prepass
        HIPCHK(hipMemcpyAsync(dst + (size_t)e->rank * count, src, count * sizeof(float), hipMemcpyDeviceToDevice, st));
        return MLGGD_OK;
    }
    NCCLCHK(g_rccl.AllGather(src, dst, count, 7 /* ncclFloat32 */, e->comm, st));
    return MLGGD_OK;
}
// The K-side factor of layer l+1 (Y_l; l = 0: the staged input rows) to the ranks that need it: every rank's rows to every
// rank (all-gather), or -- all-to-all form of the sharded update -- block p of this rank's owner-blocked Y_l to rank p,
// slot s of Yall[l] receiving rank s's block for THIS rank.  Called between gather_begin / gather_end, whose
// ncclGroupStart / End make the send / recv pairs one collective.
static int exchange_y(mlggd_engine *e, int l, const float *src, hipStream_t st = nullptr) {
    if (!e->dp_a2a) return gather_one(e, src, e->Yall[l], (size_t)e->Bp * e->lsp[l], st);
    if (e->fake_world) return MLGGD_OK;  // the emulation assembles Yall[l] per virtual owner from the sources' blocks (run_step)
    if (!st) st = e->comm_stream;
    const size_t cnt = (size_t)e->Bp * e->shard_rows[l + 1] * 64;
    for (int p = 0; p < e->world; p++) {
        NCCLCHK((int)g_rccl.Send_(src + (size_t)p * cnt, cnt, ncclFloat32, p, e->comm, st));
        NCCLCHK((int)g_rccl.Recv_(e->Yall[l] + (size_t)p * cnt, cnt, ncclFloat32, p, e->comm, st));
    }
    return MLGGD_OK;
}
// the communication stream picks up everything the main stream has produced so far (already_ordered: it has, through
// an earlier event, and nothing newer is needed -- no record / wait, i.e. no bubble on the main queue)
static int gather_begin(mlggd_engine *e, bool already_ordered = false) {
    if (!already_ordered) {
        HIPCHK(hipEventRecord(e->ev_ready, e->stream));
        HIPCHK(hipStreamWaitEvent(e->comm_stream, e->ev_ready, 0));
    }
    if (!e->fake_world) NCCLCHK(g_rccl.GroupStart());
    return MLGGD_OK;
}
static int gather_end(mlggd_engine *e) {
    if (!e->fake_world) NCCLCHK(g_rccl.GroupEnd());
    return MLGGD_OK;
}
// The next GEMM launch on the main stream produces what the communication stream is going to send: let ev_ready ride
// on that launch (see stop_ev_next).  gather_begin_armed() then only records if the launch could not take the event
// (a profiling pass owns the launch's event slots, or no GEMM launch came).
static void arm_stop(mlggd_engine *e, hipEvent_t ev) {
    if (!e->dp_stopev) return;
    e->stop_ev_next = ev;
    e->stop_ev_attached = false;
}
static bool take_stop(mlggd_engine *e) {  // true: the armed event went out with a launch
    const bool attached = e->stop_ev_next != nullptr && e->stop_ev_attached;
    e->stop_ev_next = nullptr;
    e->stop_ev_attached = false;
    return attached;
}
static void gather_arm(mlggd_engine *e) { arm_stop(e, e->ev_ready); }
static int gather_begin_armed(mlggd_engine *e) {
    if (!take_stop(e)) HIPCHK(hipEventRecord(e->ev_ready, e->stream));
    HIPCHK(hipStreamWaitEvent(e->comm_stream, e->ev_ready, 0));
    if (!e->fake_world) NCCLCHK(g_rccl.GroupStart());
    return MLGGD_OK;
}
// ---- sharded update (dp_mode 2) --------------------------------------------------------------------
// At 8 ranks the replicated dW launch is 8 x the MFMA work (298 us).  Here rank r forms only ITS block of
// weight rows of every layer over the gathered minibatch -- 1/world of the tiles -- keeps delta for that
// block only, and the updated W blocks are all-gathered in place, layer 1 first so that the next forward
// pass starts as soon as W_1 has arrived.  W is allocated with world*shard rows (zero pad rows) so that
// every rank's block has the same size.  Biases: the tiles of row block 0 run on every rank as bias-only
// jobs (no W/delta access), so all ranks apply the identical bias update without another collective.
static int shard_alloc(mlggd_engine *e) {
    for (int l = 1; l < e->L; l++) {
        const int Kp = e->lsp[l - 1], Np = e->lsp[l];
        const int k_wg = (Kp + 63) / 64;
        e->shard_rows[l] = (k_wg + e->world - 1) / e->world;
        const size_t rows = (size_t)e->shard_rows[l] * 64 * e->world;
        if (rows > (size_t)Kp) {  // grow W_l; the pad rows are never touched by a kernel (descriptors end at Kp)
            float *nw = nullptr;
            CHK(dev_alloc(e, &nw, rows * Np));
            HIPCHK(hipMemcpyAsync(nw, e->W[l], (size_t)Kp * Np * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
            e->W[l] = nw;  // the old buffer stays on the free list
            e->dwp_tables.clear();  // tile records built so far point into the old buffer
        }
        HIPCHK(hipEventCreateWithFlags(&e->ev_W[l], hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&e->ev_dw_done, hipEventDisableTiming));
    return MLGGD_OK;
}
// jobs of (virtual) rank r.  pass 0: its row blocks of every layer (own_bias: whether its own row-block-0 job
// applies the bias update); pass 1: the bias-only jobs of the layers whose row block 0 it does not own -- a
// separate launch of the bias-only kernel (k_dwp_bias)
static DwpJobs dwp_jobs_shard(mlggd_engine *e, int r, int pass, bool own_bias) {
    DwpJobs G = dwp_jobs(e, e->L - 1, 1, e->Yall[0]), J;
    memset(&J, 0, sizeof(J));
    int nj = 0, end = 0;
    {
        for (int j = 0; j < G.njobs; j++) {
            const int l = e->L - 1 - j;
            DwpArgs a = G.job[j];
            a.Yrow = e->Yall[l - 1];
            a.dEdX = e->dEdXall[l];
            const int k_wg = a.ntiles / a.n_wg;
            const int kf = r * e->shard_rows[l];
            if (e->dp_a2a) {  // Yall[l-1] holds the units of this rank's block only: [world x Bp][block width]
                a.ldA = e->shard_rows[l] * 64;
                a.k_base = pass == 0 ? kf * 64 : 0;
            }
            const int kl = kf + e->shard_rows[l] < k_wg ? kf + e->shard_rows[l] : k_wg;
            if (pass == 0 && kl > kf) {
                a.k_first = kf;
                a.ntiles = (kl - kf) * a.n_wg;
                a.do_bias = (kf == 0 && own_bias) ? 1 : 0;
            } else if (pass == 1 && kf != 0) {
                a.k_first = 0;
                a.ntiles = a.n_wg;
                a.wd_off = 1;
                a.do_bias = 1;
            } else {
                continue;
            }
            J.job[nj] = a;
            end += a.ntiles;
            J.tile_end[nj++] = end;
        }
    }
    J.njobs = nj;
    J.total = end;
    return J;
}
static DwpJobs dwp_jobs_global(mlggd_engine *e, int lhi, int llo) {
    DwpJobs J = dwp_jobs(e, lhi, llo, e->Yall[0]);
    for (int j = 0; j < J.njobs; j++) {
        const int l = lhi - j;
        J.job[j].Yrow = e->Yall[l - 1];
        J.job[j].dEdX = e->dEdXall[l];
    }
    return J;
}

static BiasJobs make_bias_jobs(mlggd_engine *e) {
    BiasJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    int first = 0, nj = 0;
    for (int l = e->L - 1; l >= 1; l--) {
        BiasJob &j = jobs.job[nj++];
        j.dEdX = e->dEdX[l];
        j.bias = e->bias[l];
        j.dbias = e->dbias[l];
        j.gb = e->gb[l];
        j.N = e->ls[l];
        j.Np = e->lsp[l];
        j.first = first;
        first += e->lsp[l];
    }
    jobs.njobs = nj;
    jobs.total = first;
    return jobs;
}

// The Adam update of one step (mlggd_set_optimizer, adam_rule.h): every layer's padded weight matrix, then every
// bias vector, in one launch.  The counters move when the launch is enqueued: a_t is the launch's argument.
static_assert(ADAM_MAXJOBS >= 2 * (MLGGD_MAXLAYER - 1), "job table too small");
static AdamJobs make_adam_jobs(mlggd_engine *e) {
    AdamJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    int nj = 0;
    unsigned first = 0;
    auto add = [&](float *w, float *m, float *v, const float *G, size_t n, float wc) {
        AdamJob &j = jobs.job[nj++];
        j.w = w, j.m = m, j.v = v, j.G = G;
        j.n4 = (unsigned)(n / 4);  // n is a multiple of 32: the padded widths are
        j.first = first;
        j.wc = wc;
        first += (j.n4 + 255u) / 256u;
    };
    for (int l = e->L - 1; l >= 1; l--)
        add(e->W[l], e->adam_mw[l].p, e->adam_vw[l].p, e->G[l], (size_t)e->lsp[l - 1] * e->lsp[l], e->cfg.weightcost);
    for (int l = e->L - 1; l >= 1; l--) add(e->bias[l], e->adam_mb[l].p, e->adam_vb[l].p, e->gb[l], (size_t)e->lsp[l], 0.0f);
    jobs.njobs = nj;
    jobs.chunks = first;
    return jobs;
}
static int run_adam_apply(mlggd_engine *e, float nf) {
    adam_rule::Products after = e->adam_prod;
    adam_rule::advance(&after, e->adam_b1, e->adam_b2);
    const adam_rule::Consts c = adam_rule::consts(nf, e->cfg.lrate, e->adam_b1, e->adam_b2, e->adam_eps, after);
    const AdamJobs jobs = make_adam_jobs(e);
    {
        ProfScope ps(e, KC_UPDATE, 1);
        hipLaunchKernelGGL(k_adam_apply, dim3(jobs.chunks > 2048u ? 2048u : jobs.chunks), dim3(256), 0, e->stream, jobs, c);
    }
    CHK(launch_check("k_adam_apply"));
    e->adam_prod = after;
    e->adam_steps++;
    return MLGGD_OK;
}

// ---- pieces of one step ----------------------------------------------------------------------------
// Where the per-dimension sum of |e|^beta of the ML loss (BP_GPU.cu:416) comes from:
enum ColsumSource {
    CS_LOCAL = 0,   // single device: every loss workgroup sums its own 32 columns of the minibatch
    CS_ALLREDUCE,   // data parallel: local sums (k_colsum), all-reduced over the communicator
    CS_GIVEN,       // e->colsum_tot already holds the global sum (one-GPU emulation of a world)
    CS_ACCUMULATE   // emulation, first pass: error + local sums only, added into e->colsum_tot; no gradient
};
// largest dynamic LDS the loss kernels are ever launched with (bunchsize 1152, the cap mlggd_create enforces)
constexpr size_t LOSS_LDS_MAX = (size_t)(32 * (1152 + 1) + 32) * sizeof(float);

// The error model in effect (ErrModel, kernels.hip.h) and the [Dp] device arrays its kernels read, nullptr where the
// model has none: the one place that knows.  Both vectors are only ever set with MLflag == 1.  EM_ASYM's shapes are the
// vector of mlggd_set_shapefactors, else cfg.shapefactor per unit.
// learn: the scale is the engine's state (mlggd_set_scale_mode, scale_rule.h) and the _learn kernels take `scale`: the
// copy this step reads, the copy it writes, the mode's parameters.  Only ever on with MLflag == 1.
struct ErrModelInUse {
    ErrModel model;
    const float *betas, *kappas;
    bool learn;
    ScaleArgs scale;
};
static ErrModelInUse err_model(const mlggd_engine *e) {
    ErrModelInUse em = {EM_SHARED, nullptr, nullptr, false, {nullptr, nullptr, 0.0f, 0.0f, 0.0f}};
    if (e->asym) em.model = EM_ASYM, em.betas = e->per_bin ? e->betas_dev : e->asym_betas_dev.p, em.kappas = e->kappas_dev.p;
    else if (e->per_bin) em.model = EM_BINS, em.betas = e->betas_dev;
    if (e->scale_mode == MLGGD_SCALE_LEARNED) {
        const size_t copy = devbuf_rule::scale_state_floats((size_t)e->Dp) / 2;
        em.learn = true;
        em.scale = {e->scale_state.p + e->scale_cur * copy, e->scale_state.p + (1 - e->scale_cur) * copy, e->scale_lrate,
                    e->scale_momentum, e->scale_vmax};
    }
    return em;
}
// One launch of a loss-family kernel: the dynamic-LDS attribute of the kernel actually launched (lds_attr 0: it needs
// none), the launch on the engine's stream, its check.
template <typename F, typename... Args>
static int launch_loss(mlggd_engine *e, const char *name, F kernel, dim3 grid, dim3 block, size_t lds_attr, size_t lds,
                       Args... args) {
    if (lds_attr) CHK(ensure_lds(e, kernel, lds_attr));
    hipLaunchKernelGGL(kernel, grid, block, lds, e->stream, args...);
    return launch_check(name);
}

// The walk of the resident chunk (inputs AND targets) that every CV-side pass makes, the bunch loop of CrossValid*
// (BP_GPU.cu:202-216): the CV forward per bunch, the trailing partial bunch INCLUDED, each followed by
// fold(bunch, its frames, its index), which launches what consumes the bunch's output slabs.
template <typename Fold>
static int walk_bunches(mlggd_engine *e, int n, Fold fold) {
    for (int i = 0, k = 0; i < n; i += e->B, k++) {
        const int fb = (e->B > n - i) ? (n - i) : e->B;
        const Bunch bn = bunch_at(e, i);
        CHK(run_forward(e, bn, fb, false));
        CHK(fold(bn, fb, k));
    }
    return MLGGD_OK;
}

// The column statistics of the resident chunk (colstats.hip.h): walk_bunches with ONE launch of `kernel` per bunch,
// which folds the bunch into `acc` (n_acc doubles, allocated on first use; fresh: the first bunch overwrites); one
// download of `rows` rows and one synchronise.
template <class Args>
static int col_stats_resident(mlggd_engine *e, int n, DevBuf<double> &acc, size_t n_acc, int rows, void (*kernel)(Args),
                              const char *name, Args a, double *sums) {
    HIPCHK(acc.grow(n_acc, n_acc, e->bufs, nullptr, nullptr));
    a.slab = e->slab; a.S = e->S_out; a.bias = e->bias[e->L - 1];
    a.D = e->D; a.Dp = e->Dp; a.Bp = e->Bp; a.toff = e->toff; a.acc = acc.p;
    CHK(walk_bunches(e, n, [&](const Bunch &bn, int fb, int k) {
        a.targ = bn.targ; a.first = bn.first; a.B = fb; a.fresh = k == 0;
        hipLaunchKernelGGL(kernel, dim3(e->Dp / COLSTATS_DT), dim3(256), 0, e->stream, a);
        return launch_check(name);
    }));
    HIPCHK(hipMemcpyAsync(sums, acc.p, (size_t)rows * e->D * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}

// Output-layer loss of one minibatch: BP_GPU.cu:408-423.  sa / n_stage: input-staging blocks of the NEXT
// minibatch that ride along with the first loss launch (n_stage 0: none).
static int run_loss(mlggd_engine *e, const Bunch &bn, float nf, float inv_n, ColsumSource cs, bool first_acc,
                    const StageArgs &sa, int n_stage) {
    const int L = e->L, B = e->B, Bp = e->Bp, b_tiles = Bp / 32, ML = e->cfg.MLflag;
    const ErrModelInUse em = err_model(e);
    ProfScope ps(e, KC_LOSS, 0);
    const size_t lds_grad = (size_t)(LOSS_DT * (Bp + 1) + LOSS_DT) * sizeof(float);  // k_loss_grad: LOSS_DT columns
    const int n_loss = (e->Dp / LOSS_DT) * b_tiles;  // 8 (d) x 32 (b) elements per loss workgroup, one per thread
    if (ML != 1 && e->loss_fuse) {
        if (cs == CS_ACCUMULATE) return MLGGD_OK;  // no minibatch statistic without the ML loss
        LossNormArgs la;
        la.slab = e->slab; la.S = e->S_out; la.bias = e->bias[L - 1]; la.targ = bn.targ;
        la.B = B; la.D = e->D; la.Dp = e->Dp; la.Bp = Bp; la.beta = e->cfg.shapefactor; la.inv_n = inv_n;
        la.outT = e->outT; la.eT = e->eT; la.dEdXt = e->dEdXt[L - 1]; la.dEdX = e->dEdX[L - 1];
        la.b_tiles = b_tiles; la.first = bn.first; la.toff = e->toff;
        hipLaunchKernelGGL(k_loss_norm, dim3(n_loss + n_stage), dim3(256), 0, e->stream, la, n_loss, sa);
        return launch_check("k_loss_norm");
    }
    if (ML == 1 && cs == CS_LOCAL && e->loss_fuse) {  // single device: the whole ML loss in one launch
        LossMlArgs la;
        la.slab = e->slab; la.S = e->S_out; la.bias = e->bias[L - 1]; la.targ = bn.targ;
        la.B = B; la.D = e->D; la.Dp = e->Dp; la.Bp = Bp; la.beta = e->cfg.shapefactor; la.nf = nf; la.inv_n = inv_n;
        la.outT = e->outT; la.eT = e->eT; la.scalefactor = e->scalefactor; la.dEdXt = e->dEdXt[L - 1]; la.dEdX = e->dEdX[L - 1];
        la.first = bn.first; la.toff = e->toff;
        const size_t lds_ml = (size_t)2 * LOSS_DT * (Bp + 1) * sizeof(float);
        const size_t lds_ml_max = (size_t)2 * LOSS_DT * (1152 + 1) * sizeof(float);
        const int n_ml = e->Dp / LOSS_DT;
        const dim3 grid(n_ml + (n_stage + 3) / 4), block(1024);
        if (em.learn) switch (em.model) {
            case EM_ASYM:
                return launch_loss(e, "k_loss_ml_learn_asym", k_loss_ml_learn_asym, grid, block, lds_ml_max, lds_ml, la, em.scale,
                                   em.betas, em.kappas, n_ml, sa, n_stage);
            case EM_BINS:
                return launch_loss(e, "k_loss_ml_learn_bins", k_loss_ml_learn_bins, grid, block, lds_ml_max, lds_ml, la, em.scale,
                                   em.betas, n_ml, sa, n_stage);
            default:
                return launch_loss(e, "k_loss_ml_learn", k_loss_ml_learn, grid, block, lds_ml_max, lds_ml, la, em.scale, n_ml, sa,
                                   n_stage);
            }
        switch (em.model) {
        case EM_ASYM:
            return launch_loss(e, "k_loss_ml_asym", k_loss_ml_asym, grid, block, lds_ml_max, lds_ml, la, em.betas, em.kappas,
                               n_ml, sa, n_stage);
        case EM_BINS:
            return launch_loss(e, "k_loss_ml_bins", k_loss_ml_bins, grid, block, lds_ml_max, lds_ml, la, em.betas, n_ml, sa,
                               n_stage);
        default:
            return launch_loss(e, "k_loss_ml", k_loss_ml, grid, block, lds_ml_max, lds_ml, la, n_ml, sa, n_stage);
        }
    }
    LossErrArgs la;
    la.slab = e->slab; la.S = e->S_out; la.bias = e->bias[L - 1]; la.targ = bn.targ;
    la.B = B; la.D = e->D; la.Dp = e->Dp; la.Bp = Bp; la.beta = e->cfg.shapefactor; la.want_pow = ML == 1 ? 1 : 0;
    la.outT = e->outT; la.eT = e->eT; la.pT = e->pT;
    la.b_tiles = b_tiles; la.first = bn.first; la.toff = e->toff;
    const dim3 grid_err(n_loss + n_stage), grid(n_loss), block(256);
    switch (em.model) {
    case EM_ASYM:
        CHK(launch_loss(e, "k_loss_err_asym", k_loss_err_asym, grid_err, block, 0, 0, la, em.betas, em.kappas, n_loss, sa));
        break;
    case EM_BINS:
        CHK(launch_loss(e, "k_loss_err_bins", k_loss_err_bins, grid_err, block, 0, 0, la, em.betas, n_loss, sa));
        break;
    default:
        CHK(launch_loss(e, "k_loss_err", k_loss_err, grid_err, block, 0, 0, la, n_loss, sa));
    }
    const float *colsum_in = nullptr;
    if (ML == 1 && cs == CS_GIVEN) {
        colsum_in = e->colsum_tot;
    } else if (ML == 1 && cs != CS_LOCAL) {
        hipLaunchKernelGGL(k_colsum, dim3(e->Dp / 32), dim3(256), 0, e->stream, e->pT, B, Bp, e->colsum);  // wavefront reductions
        CHK(launch_check("k_colsum"));
        if (cs == CS_ACCUMULATE) {
            hipLaunchKernelGGL(k_accum, dim3(1), dim3(256), 0, e->stream, e->colsum_tot,
                               first_acc ? (const float *)nullptr : (const float *)e->colsum_tot, (const float *)e->colsum,
                               (size_t)e->Dp);
            return launch_check("k_accum");
        }
        NCCLCHK(g_rccl.AllReduce(e->colsum, e->colsum, (size_t)e->Dp, 7, 0, e->stat_comm ? e->stat_comm : e->comm, e->stream));
        colsum_in = e->colsum;
    }
    if (cs == CS_ACCUMULATE) return MLGGD_OK;
    float *const dEdXt = e->dEdXt[L - 1], *const dEdX = e->dEdX[L - 1];
    if (em.learn) switch (em.model) {
        case EM_ASYM:
            return launch_loss(e, "k_loss_grad_learn_asym", k_loss_grad_learn_asym, grid, block, LOSS_LDS_MAX, lds_grad, e->eT,
                               e->pT, colsum_in, B, e->D, e->Dp, Bp, em.betas, em.kappas, nf, inv_n, e->scalefactor, dEdXt, dEdX,
                               b_tiles, em.scale);
        case EM_BINS:
            return launch_loss(e, "k_loss_grad_learn_bins", k_loss_grad_learn_bins, grid, block, LOSS_LDS_MAX, lds_grad, e->eT,
                               e->pT, colsum_in, B, e->D, e->Dp, Bp, em.betas, nf, inv_n, e->scalefactor, dEdXt, dEdX, b_tiles,
                               em.scale);
        default:
            return launch_loss(e, "k_loss_grad_learn", k_loss_grad_learn, grid, block, LOSS_LDS_MAX, lds_grad, e->eT, e->pT,
                               colsum_in, B, e->D, e->Dp, Bp, e->cfg.shapefactor, nf, inv_n, e->scalefactor, dEdXt, dEdX, b_tiles,
                               em.scale);
        }
    switch (em.model) {
    case EM_ASYM:
        return launch_loss(e, "k_loss_grad_asym", k_loss_grad_asym, grid, block, LOSS_LDS_MAX, lds_grad, e->eT, e->pT,
                           colsum_in, B, e->D, e->Dp, Bp, em.betas, em.kappas, nf, inv_n, e->scalefactor, dEdXt, dEdX, b_tiles);
    case EM_BINS:
        return launch_loss(e, "k_loss_grad_bins", k_loss_grad_bins, grid, block, LOSS_LDS_MAX, lds_grad, e->eT, e->pT,
                           colsum_in, B, e->D, e->Dp, Bp, em.betas, nf, inv_n, e->scalefactor, dEdXt, dEdX, b_tiles);
    default:
        return launch_loss(e, "k_loss_grad", k_loss_grad, grid, block, LOSS_LDS_MAX, lds_grad, e->eT, e->pT, colsum_in, B,
                           e->D, e->Dp, Bp, e->cfg.shapefactor, ML, nf, inv_n, e->scalefactor, dEdXt, dEdX, b_tiles);
    }
}

// a 32 x 32-tile dX launch in the form PIPE (dx_dma); the stamped instantiation only when the launch was picked for stamps
template <int PIPE, int ACT>
static int launch_dx(mlggd_engine *e, int nwg, const DxArgs &xa, long long *st) {
    const size_t lds = dx_lds_floats<4, PIPE>() * sizeof(float);
    if (st) {
        CHK(ensure_lds(e, k_dx<4, PIPE, ACT, true>, lds));
        launch_timed(e, k_dx<4, PIPE, ACT, true>, dim3(nwg), dim3(256), lds, e->stream, xa, st);
    } else {
        CHK(ensure_lds(e, k_dx<4, PIPE, ACT, false>, lds));
        launch_timed(e, k_dx<4, PIPE, ACT, false>, dim3(nwg), dim3(256), lds, e->stream, xa, st);
    }
    return MLGGD_OK;
}

// dEdX_{l-1} from dEdX_l and the OLD W_l (+ the derivative of layer l-1's activation): BP_GPU.cu:402,430
static int run_dx(mlggd_engine *e, int l) {
    const int Kp = e->lsp[l - 1], b_tiles = e->Bp / 32;
    const bool relu = e->cfg.activation == MLGGD_ACT_RELU;
    ProfScope ps(e, KC_DX, l);
    DxArgs xa = dx_args(e, l);
    if (dx64_used(e, l)) {
        xa.k_tiles = Kp / 64;
        xa.b_tiles = e->Bp / 64;
        xa.b_shift = log2_or_minus1(xa.b_tiles);
        const size_t lds = t64_lds_floats() * sizeof(float);
        if (relu) {
            CHK(ensure_lds(e, k_dx64<ACT_RELU>, lds));
            launch_timed(e, k_dx64<ACT_RELU>, dim3(xa.k_tiles * xa.b_tiles), dim3(256), lds, e->stream, xa);
        } else {
            CHK(ensure_lds(e, k_dx64<ACT_SIGMOID>, lds));
            launch_timed(e, k_dx64<ACT_SIGMOID>, dim3(xa.k_tiles * xa.b_tiles), dim3(256), lds, e->stream, xa);
        }
        return launch_check("k_dx64");
    }
    long long *st = stamps_for(e, KC_DX, l, (Kp / 32) * b_tiles);  // k_dx64 carries no stamps: it leaves the selection alone
    const int nwg = (Kp / 32) * b_tiles;
    if (dx_dma(e, Kp)) CHK((relu ? launch_dx<4, ACT_RELU>(e, nwg, xa, st) : launch_dx<4, ACT_SIGMOID>(e, nwg, xa, st)));
    else CHK((relu ? launch_dx<1, ACT_RELU>(e, nwg, xa, st) : launch_dx<1, ACT_SIGMOID>(e, nwg, xa, st)));
    return launch_check("k_dx");
}

// the weight-gradient kernel of ONE layer (fused: with the update as its epilogue; else G_l, gb_l are written)
static int launch_dw_layer(mlggd_engine *e, int l, const float *in_rows, bool fused, float nf) {
    const int Kp = e->lsp[l - 1], Np = e->lsp[l];
    const long tiles128 = (long)((Kp + 127) / 128) * ((Np + 127) / 128);
    const bool big = e->dw_tile == 0 ? tiles128 >= 192 : e->dw_tile == 2;
    ProfScope ps(e, KC_DW, l);
    if (dwp_usable(e)) return launch_dwp(e, dwp_jobs(e, l, l, in_rows), dwp_const(e, nf, e->B), fused, l);
    if (big) return launch_dw<2>(e, l, in_rows, fused, nf);
    return launch_dw<1>(e, l, in_rows, fused, nf);
}

static int launch_accum(float *dst, const float *a, const float *b, size_t n, hipStream_t st) {
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_accum, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, st, dst, a, b, n);
    return launch_check("k_accum");
}

// One-GPU emulation of a world of ranks (mlggd_debug_fake_world).  The global minibatch is rows
// [sample0, sample0 + world*B) of the resident chunk and emulated rank r owns rows [sample0 + r*B, +B) of it:
// the partition of SURVEY 8e, with DIFFERENT rows on every rank.  Ranks 0 .. world-2 run here, one after the
// other, and leave behind what the collectives would have delivered: the ML statistic of ALL ranks in
// colsum_tot, their factors in slot r of Yall / dEdXall (gather modes), or their gradients summed into
// Gpre / gbpre (all-reduce mode).  The last rank then takes the real data-parallel path of run_step with
// device copies / adds in place of the RCCL calls.
// floats of Y_l (l = 0: the staged input rows) as the producers write it: [Bp][lsp[l]], or -- all-to-all form -- owner-
// blocked, world blocks of [Bp][block width of layer l+1]
static size_t y_count(const mlggd_engine *e, int l) {
    return e->dp_a2a ? (size_t)e->world * e->Bp * e->shard_rows[l + 1] * 64 : (size_t)e->Bp * e->lsp[l];
}
static int keep_alloc(mlggd_engine *e) {
    if (!e->keep_ranks || !e->fake_world || !e->snap_x.empty()) return MLGGD_OK;
    for (int r = 0; r + 1 < e->world; r++) {
        float *p = nullptr;
        CHK(dev_alloc(e, &p, y_count(e, 0)));
        e->snap_x.push_back(p);
        CHK(dev_alloc(e, &p, (size_t)e->Dp * e->Bp));
        e->snap_out.push_back(p);
        for (int l = 1; l < e->L; l++) {
            if (l < e->L - 1) {
                CHK(dev_alloc(e, &p, y_count(e, l)));
                e->snap_y[l].push_back(p);
            }
            CHK(dev_alloc(e, &p, (size_t)e->Bp * e->lsp[l]));
            e->snap_dedx[l].push_back(p);
        }
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}
// emulated rank r's step is complete up to dW: its factors and output, device to device on the engine's stream
static int keep_snapshot(mlggd_engine *e, int r, const float *in_rows) {
    auto cp = [&](float *dst, const float *src, size_t count) -> int {
        HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
        return MLGGD_OK;
    };
    CHK(cp(e->snap_x[r], in_rows, y_count(e, 0)));
    CHK(cp(e->snap_out[r], e->outT, (size_t)e->Dp * e->Bp));
    for (int l = 1; l < e->L; l++) {
        if (l < e->L - 1) CHK(cp(e->snap_y[l][r], e->Y[l], y_count(e, l)));
        CHK(cp(e->snap_dedx[l][r], e->dEdX[l], (size_t)e->Bp * e->lsp[l]));
    }
    return MLGGD_OK;
}

static int fake_world_prepass(mlggd_engine *e, int sample0, float nf, float inv_n) {
    const int L = e->L, B = e->B, Bp = e->Bp, W = e->world;
    StageArgs none;
    memset(&none, 0, sizeof(none));
    if (e->cfg.MLflag == 1)
        for (int r = 0; r < W; r++) {
            const Bunch bn = bunch_at(e, sample0 + r * B);
            CHK(run_forward(e, bn, B, true));
            CHK(run_loss(e, bn, nf, inv_n, CS_ACCUMULATE, r == 0, none, 0));
        }
    for (int r = 0; r + 1 < W; r++) {
        const Bunch bn = bunch_at(e, sample0 + r * B);
        CHK(run_forward(e, bn, B, true));
        const float *in_rows = bunch_rows(e, bn);
        CHK(run_loss(e, bn, nf, inv_n, CS_GIVEN, false, none, 0));
        for (int l = L - 1; l >= 2; l--) CHK(run_dx(e, l));
        if (e->keep_ranks) CHK(keep_snapshot(e, r, in_rows));
        if (e->dp_mode >= 1) {
            auto put = [&](const float *src, float *dst, size_t count) -> int {
                HIPCHK(hipMemcpyAsync(dst + (size_t)r * count, src, count * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
                return MLGGD_OK;
            };
            if (e->dp_a2a) {  // keep source r's owner-blocked factors whole: every virtual owner picks its block later
                for (int l = 0; l < L - 1; l++) {
                    const size_t all = (size_t)e->world * Bp * e->shard_rows[l + 1] * 64;
                    HIPCHK(hipMemcpyAsync(e->Ysrc[l][r], l == 0 ? in_rows : e->Y[l], all * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
                }
            } else {
                CHK(put(in_rows, e->Yall[0], (size_t)Bp * e->lsp[0]));
                for (int l = 1; l < L - 1; l++) CHK(put(e->Y[l], e->Yall[l], (size_t)Bp * e->lsp[l]));
            }
            for (int l = 1; l < L; l++) CHK(put(e->dEdX[l], e->dEdXall[l], (size_t)Bp * e->lsp[l]));
        } else {
            for (int l = L - 1; l >= 1; l--) {
                CHK(launch_dw_layer(e, l, in_rows, false, nf));
                CHK(launch_accum(e->Gpre[l], r == 0 ? nullptr : e->Gpre[l], e->G[l], (size_t)e->lsp[l - 1] * e->lsp[l], e->stream));
            }
            CHK(launch_accum(e->gbpre, r == 0 ? nullptr : e->gbpre, e->gb_all, e->gb_all_count, e->stream));
        }
    }
    return MLGGD_OK;
}

// One SGD step on `frames` (= bunchsize) resident frames: BP_GPU::train_bunch_single,
// BP_GPU.cu:308-440.
// next != nullptr: also stage that bunch's input for the following step (its blocks ride along
// with the loss kernel; see k_loss_norm).  prestaged: this bunch was staged that way.
// sample0: index of the minibatch's first row in the resident chunk (only the emulated world needs it).
static int run_step(mlggd_engine *e, int sample0, bool prestaged = false, const Bunch *next = nullptr) {
    const int L = e->L, B = e->B, Bp = e->Bp;
    e->stop_ev_next = nullptr;  // see run_forward
    e->stop_ev_attached = false;
    const bool dp = e->comm != nullptr || e->fake_world;  // a 1-rank communicator still takes the exchange path (tests)
    const bool gather = dp && e->dp_mode >= 1;
    const int n_global = B * e->world;
    const float nf = (float)n_global;
    const float inv_n = 1.0f / n_global;  // DevVecMulNum(..., 1.0f/n_frames, ...), BP_GPU.cu:409,423
    const int ML = e->cfg.MLflag;
    if (e->fake_world) {
        CHK(fake_world_prepass(e, sample0, nf, inv_n));
        sample0 += (e->world - 1) * B;  // the last emulated rank runs below
    }
    const Bunch bn = bunch_at(e, sample0);
    RoctxRange step_range("mlggd step");

    // With the ML loss the hidden activations are sent AFTER the loss kernels: the 257-float all-reduce of the
    // loss statistic uses the same communicator, and collectives of one communicator run one after the other
    // whatever stream they are on -- it must not queue behind megabytes of factors (the input rows, sent at
    // the start of the step, have long arrived by then).
    // fine: replicated update on few ranks -- send every factor as soon as it exists (the links are the
    // bottleneck there, so they should never idle) and start the upper layers' dW while dEdX_1 still travels
    const bool fine = gather && e->dp_mode == 1 && e->dp_fine != 0;
    {
        RoctxRange r("forward");
        CHK(run_forward(e, bn, B, true, prestaged,
                        gather ? (GATHER_INPUT | (ML != 1 ? (fine ? GATHER_HIDDEN_EACH : GATHER_HIDDEN) : 0)) : 0));
    }
    const float *in_rows = bunch_rows(e, bn);  // after run_forward: it may have switched in_bunch
    // input of the next step: Yt[0] is free from here on (forward_1 has been enqueued); frame-stream
    // rows go to the OTHER in_bunch buffer because this step's dW(1) still reads the current one
    StageArgs sa;
    memset(&sa, 0, sizeof(sa));
    int n_stage = 0;
    if (next) {
        sa = stage_args(e, *next, B, in_bunch_other(e));
        n_stage = stage_blocks(e);
    }
    {
        RoctxRange r("loss (+ staging of the next minibatch)");
        CHK(run_loss(e, bn, nf, inv_n, !dp ? CS_LOCAL : e->fake_world ? CS_GIVEN : CS_ALLREDUCE, false, sa, n_stage));
        // the learned scale: every loss launch of this step (one per emulated rank, the prepass included) has read copy
        // scale_cur and written the other; the next step reads what they wrote
        if (e->scale_mode == MLGGD_SCALE_LEARNED) e->scale_cur ^= 1, e->scale_steps++;
    }
    RoctxRange back_range("backward: dX, dW + update, exchange");
    if (gather && ML == 1 && L > 2) {
        CHK(gather_begin(e));
        for (int g = 1; g < L - 1; g++) CHK(exchange_y(e, g, e->Y[g], nullptr));
        CHK(gather_end(e));
    }
    // single GPU: every dW(l) only needs dEdX_l and Y_{l-1}, so one persistent launch walks the
    // tiles of all layers after the last dX (the data-parallel path keeps one launch per layer so
    // that the all-reduce of layer l overlaps the rest of the backward pass)
    // Adam (single device only): the dW launches of the all-reduce exchange, unfused and one per layer, write G_l / gb_l
    // and k_adam_apply ends the step
    const bool adam = e->opt_kind == MLGGD_OPT_ADAM;
    const bool merged = (!dp && !adam && e->dw_merge && dwp_usable(e)) || gather;
    int pending_hi = L - 1;  // gather mode: dEdX_l for l in [l .. pending_hi] are final and not yet sent
    bool mainline_done = false;  // the last factor group went out on the main stream: the dW launch needs no further event
    for (int l = L - 1; l >= 1; l--) {
        const int Kp = e->lsp[l - 1], Np = e->lsp[l];
        if (fine) {  // dEdX_l is final here (loss or dX_{l+1} has been enqueued): send it, layer l is then complete
            CHK(gather_begin_armed(e));  // the event rode on dX_{l+1}'s launch (armed below), else it is recorded here
            CHK(gather_one(e, e->dEdX[l], e->dEdXall[l], (size_t)Bp * e->lsp[l]));
            CHK(gather_end(e));
            HIPCHK(hipEventRecord(e->ev_layer[l], e->comm_stream));
        } else if (gather && l <= 2) {  // two groups: everything down to dEdX_2 beside dX_2, dEdX_1 at the end
            if (l == 1 && e->dp_mainline) {
                // dEdX_1 is the one factor nothing can hide: the dW launch waits for it.  On the MAIN stream it costs
                // its own time; by way of the communication stream it cost two event hand-offs more (30 us between
                // dX_2 and k_dwp in the 1-rank rehearsal).  The earlier groups are awaited here, where they have
                // long arrived.
                HIPCHK(hipEventRecord(e->ev_gathered, e->comm_stream));
                HIPCHK(hipStreamWaitEvent(e->stream, e->ev_gathered, 0));
                if (!e->fake_world) NCCLCHK(g_rccl.GroupStart());
                for (int g = pending_hi; g >= l; g--)
                    CHK(gather_one(e, e->dEdX[g], e->dEdXall[g], (size_t)Bp * e->lsp[g], e->stream));
                if (!e->fake_world) NCCLCHK(g_rccl.GroupEnd());
                mainline_done = true;
            } else {
                CHK(gather_begin_armed(e));
                for (int g = pending_hi; g >= l; g--) CHK(gather_one(e, e->dEdX[g], e->dEdXall[g], (size_t)Bp * e->lsp[g]));
                CHK(gather_end(e));
            }
            pending_hi = l - 1;
        }
        // dX_l produces dEdX_{l-1}; if the next iteration sends it (or a group ending with it) on the communication
        // stream, the event that stream waits for rides on this launch
        if (l != 1 && gather && (fine || l - 1 == 2 || (l - 1 == 1 && !e->dp_mainline))) gather_arm(e);
        if (l != 1) CHK(run_dx(e, l));
        if (merged) continue;  // all layers' dW + update run as one launch after the last dX
        if (dp && !gather) arm_stop(e, e->ev_grad[l]);  // "G_l written" rides on the launch that writes it
        CHK(launch_dw_layer(e, l, in_rows, !dp && !adam, nf));
        if (dp && !gather) {
            if (!take_stop(e)) HIPCHK(hipEventRecord(e->ev_grad[l], e->stream));
            HIPCHK(hipStreamWaitEvent(e->comm_stream, e->ev_grad[l], 0));
            if (e->fake_world) {  // sum over the emulated ranks: what the all-reduce (or the union of the reduce-scatter blocks) delivers
                if (e->world > 1) CHK(launch_accum(e->G[l], e->Gpre[l], e->G[l], (size_t)Kp * Np, e->comm_stream));
            } else if (e->ar_shard) {
                // reduce-scatter over blocks of weight rows (shard_rows[l] tile rows of 64 per rank; G_l is allocated
                // with world x block rows, the rows past Kp stay zero): this rank receives the sum of ITS block, in place
                const size_t blk = (size_t)e->shard_rows[l] * 64 * Np;
                NCCLCHK(g_rccl.ReduceScatter(e->G[l], e->G[l] + (size_t)e->rank * blk, blk, e->comm, e->comm_stream));
            } else {
                NCCLCHK(g_rccl.AllReduce(e->G[l], e->G[l], (size_t)Kp * Np, 7, 0, e->comm, e->comm_stream));
            }
            HIPCHK(hipEventRecord(e->ev_red[l], e->comm_stream));
        }
    }
    if (gather && e->dp_mode == 2) {
        if (!mainline_done) {
            HIPCHK(hipEventRecord(e->ev_gathered, e->comm_stream));
            HIPCHK(hipStreamWaitEvent(e->stream, e->ev_gathered, 0));
        }
        const int units = e->world * Bp / 64;
        const DwpConst C = dwp_const(e, nf, e->world * Bp);
        if (e->fake_world) {
            // all virtual ranks in turn on this GPU: their row blocks are disjoint, so the union is the whole
            // update; the bias update is taken from the LAST rank's bias-only jobs so that path is exercised
            const char *only = getenv("MLGGD_FAKE_ONLY_RANK");  // timing: run one rank's share only (tools/dp_sim.py)
            for (int r = 0; r < e->world; r++) {
                if (only && atoi(only) != r) continue;
                if (e->dp_a2a)  // what the all-to-all delivers to virtual owner r: its block of every source's Y_l
                    for (int l = 0; l < L - 1; l++) {
                        const size_t cnt = (size_t)Bp * e->shard_rows[l + 1] * 64;
                        for (int sr = 0; sr < e->world; sr++) {
                            const float *src = sr + 1 < e->world ? e->Ysrc[l][sr] : (l == 0 ? in_rows : e->Y[l]);
                            HIPCHK(hipMemcpyAsync(e->Yall[l] + (size_t)sr * cnt, src + (size_t)r * cnt, cnt * sizeof(float),
                                                  hipMemcpyDeviceToDevice, e->stream));
                        }
                    }
                if (only || r == e->world - 1) {  // the bias update comes from the LAST rank's bias-only tiles
                    DwpJobs Jb = dwp_jobs_shard(e, r, 1, false);
                    if (Jb.total > 0) CHK(launch_dwp(e, Jb, C, true, 1, units));
                }
                DwpJobs J = dwp_jobs_shard(e, r, 0, only ? true : e->world == 1);
                ProfScope ps(e, KC_DW, 1);
                if (J.total > 0) CHK(launch_dwp(e, J, C, true, 1, units));
            }
        } else {
            {
                DwpJobs Jb = dwp_jobs_shard(e, e->rank, 1, false);  // bias-only tiles: no W access, so they go first
                if (Jb.total > 0) CHK(launch_dwp(e, Jb, C, true, 1, units));
                ProfScope ps(e, KC_DW, 1);
                DwpJobs J = dwp_jobs_shard(e, e->rank, 0, true);
                arm_stop(e, e->ev_dw_done);  // the event the W gathers wait for rides on this launch
                if (J.total > 0) CHK(launch_dwp(e, J, C, true, 1, units));
            }
            const bool dw_done_attached = take_stop(e);
            // W_1 is what the next forward pass waits for first: its all-gather goes on the MAIN stream, right behind
            // the update (no hand-off to the communication stream and back: 21 us between k_dwp and forward_1 in the
            // 1-rank rehearsal); the upper layers' blocks travel on the communication stream beside forward_1
            if (!dw_done_attached) HIPCHK(hipEventRecord(e->ev_dw_done, e->stream));
            HIPCHK(hipStreamWaitEvent(e->comm_stream, e->ev_dw_done, 0));
            e->comm_after_dw = true;
            for (int l = 1; l < L; l++) {  // layer 1 first: the next forward pass needs it first
                const size_t count = (size_t)e->shard_rows[l] * 64 * e->lsp[l];
                hipStream_t st = (l == 1 && e->dp_mainline) ? e->stream : e->comm_stream;
                NCCLCHK(g_rccl.AllGather(e->W[l] + (size_t)e->rank * count, e->W[l], count, 7, e->comm, st));
                if (st == e->comm_stream) {
                    HIPCHK(hipEventRecord(e->ev_W[l], e->comm_stream));
                    e->ev_W_pending[l] = true;
                }
            }
        }
    } else if (fine) {
        // two launches: layers L-1..2 as soon as dEdX_2 has arrived (after dX_2 in stream order, which still reads
        // the old W_2), layer 1 when dEdX_1 has
        const int units = e->world * Bp / 64;
        const DwpConst C = dwp_const(e, nf, e->world * Bp);
        if (L - 1 >= 2) {
            HIPCHK(hipStreamWaitEvent(e->stream, e->ev_layer[2], 0));
            ProfScope ps(e, KC_DW, L - 1);
            CHK(launch_dwp(e, dwp_jobs_global(e, L - 1, 2), C, true, L - 1, units));
        }
        HIPCHK(hipStreamWaitEvent(e->stream, e->ev_layer[1], 0));
        ProfScope ps(e, KC_DW, 1);
        CHK(launch_dwp(e, dwp_jobs_global(e, 1, 1), C, true, 1, units));
    } else if (gather) {
        if (!mainline_done) {
            HIPCHK(hipEventRecord(e->ev_gathered, e->comm_stream));
            HIPCHK(hipStreamWaitEvent(e->stream, e->ev_gathered, 0));
        }
        ProfScope ps(e, KC_DW, 1);
        CHK(launch_dwp(e, dwp_jobs_global(e, L - 1, 1), dwp_const(e, nf, e->world * Bp), true, 1, e->world * Bp / 64));
    } else if (merged) {
        ProfScope ps(e, KC_DW, 1);
        CHK(launch_dwp(e, dwp_jobs(e, L - 1, 1, in_rows), dwp_const(e, nf, e->B), true, 1));
    }
    if (dp && !gather) {
        // bias gradients were written by the dw kernels; ev_grad[1] is the last of them
        HIPCHK(hipStreamWaitEvent(e->comm_stream, e->ev_grad[1], 0));
        if (e->fake_world) {
            if (e->world > 1) CHK(launch_accum(e->gb_all, e->gbpre, e->gb_all, e->gb_all_count, e->comm_stream));
        } else {
            NCCLCHK(g_rccl.AllReduce(e->gb_all, e->gb_all, e->gb_all_count, 7, 0, e->comm, e->comm_stream));
        }
        HIPCHK(hipEventRecord(e->ev_bias_red, e->comm_stream));
        for (int l = L - 1; l >= 1; l--) {
            HIPCHK(hipStreamWaitEvent(e->stream, e->ev_red[l], 0));
            ProfScope ps(e, KC_UPDATE, l);
            const int Kp = e->lsp[l - 1], Np = e->lsp[l];
            // kernUpdatedelta + kernAccSum (DevFunc.cu:490-507,427-443) on the rows [row0, row0 + rows) of W_l: the
            // whole matrix (MLGGD_DP_AR_SHARD=0), or the block of weight rows this rank received the summed gradient
            // of -- delta is kept for that block only.  The emulated world has every block's sum in G_l and applies
            // the blocks of all its ranks one after the other (they are disjoint: the union is the whole update).
            const int r_lo = !e->ar_shard ? 0 : e->fake_world ? 0 : e->rank;
            const int r_hi = !e->ar_shard ? 0 : e->fake_world ? e->world - 1 : e->rank;
            const char *only = e->fake_world ? getenv("MLGGD_FAKE_ONLY_RANK") : nullptr;  // timing: one rank's share only (tools/dp_sim.py)
            for (int r = r_lo; r <= r_hi; r++) {
                if (only && e->ar_shard && atoi(only) != r) continue;
                const int row0 = e->ar_shard ? r * e->shard_rows[l] * 64 : 0;
                const int row1 = e->ar_shard ? (row0 + e->shard_rows[l] * 64 < Kp ? row0 + e->shard_rows[l] * 64 : Kp) : Kp;
                if (row1 <= row0) continue;  // a block that lies entirely in the pad rows
                const size_t off = (size_t)row0 * Np, n4 = (size_t)(row1 - row0) * Np / 4;
                const size_t blocks = (n4 + 255) / 256;
                hipLaunchKernelGGL(k_apply_update, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, e->stream,
                                   e->W[l] + off, e->dW[l] + off, e->G[l] + off, n4, nf, e->cfg.momentum, e->cfg.lrate,
                                   e->cfg.weightcost);
                CHK(launch_check("k_apply_update"));
            }
        }
        HIPCHK(hipStreamWaitEvent(e->stream, e->ev_bias_red, 0));
        BiasJobs jobs = make_bias_jobs(e);
        hipLaunchKernelGGL(k_bias_apply, dim3((jobs.total + 255) / 256), dim3(256), 0, e->stream, jobs, nf,
                           e->cfg.momentum, e->cfg.lrate);
        CHK(launch_check("k_bias_apply"));
        if (e->ar_shard && !e->fake_world) {
            // the updated W blocks travel back: all-gather in place, layer 1 first and -- like the sharded factor
            // mode -- on the MAIN stream (the next forward pass waits for it first; no hand-off to the communication
            // stream and back), the upper layers on the communication stream beside forward_1, each with its event
            HIPCHK(hipEventRecord(e->ev_dw_done, e->stream));
            HIPCHK(hipStreamWaitEvent(e->comm_stream, e->ev_dw_done, 0));
            for (int l = 1; l < L; l++) {
                const size_t count = (size_t)e->shard_rows[l] * 64 * e->lsp[l];
                hipStream_t st = (l == 1 && e->dp_mainline) ? e->stream : e->comm_stream;
                NCCLCHK(g_rccl.AllGather(e->W[l] + (size_t)e->rank * count, e->W[l], count, 7, e->comm, st));
                if (st == e->comm_stream) {
                    HIPCHK(hipEventRecord(e->ev_W[l], e->comm_stream));
                    e->ev_W_pending[l] = true;
                }
            }
        }
    }
    if (adam) CHK(run_adam_apply(e, nf));
    e->step_counter++;
    return MLGGD_OK;
}

static int create_concurrent_stream(mlggd_engine *e, hipStream_t *out, const char *what);

// ------------------------------------------------------------------ C-ABI
extern "C" {

const char *mlggd_last_error(void) { return g_err; }

int mlggd_device_count(int *count) {
    if (!count) return fail(MLGGD_ERR_ARG, "count is NULL");
    HIPCHK(hipGetDeviceCount(count));
    return MLGGD_OK;
}

int mlggd_create(const mlggd_config *cfg, const float *const *weights, const float *const *bias, mlggd_handle *out) {
    if (!cfg || !weights || !bias || !out) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (cfg->struct_size != (int32_t)sizeof(mlggd_config))
        return fail(MLGGD_ERR_ARG, "mlggd_config.struct_size %d != %d", cfg->struct_size, (int)sizeof(mlggd_config));
    if (cfg->numlayers < 2 || cfg->numlayers > MLGGD_MAXLAYER)
        return fail(MLGGD_ERR_ARG, "numlayers %d not in 2..%d", cfg->numlayers, MLGGD_MAXLAYER);
    if (cfg->bunchsize < 1) return fail(MLGGD_ERR_ARG, "bunchsize %d < 1", cfg->bunchsize);
    if (cfg->activation != MLGGD_ACT_SIGMOID && cfg->activation != MLGGD_ACT_RELU)
        return fail(MLGGD_ERR_ARG, "activation %d: must be %d (sigmoid) or %d (relu)", cfg->activation, MLGGD_ACT_SIGMOID,
                    MLGGD_ACT_RELU);
    if (cfg->nat_frames < 0) return fail(MLGGD_ERR_ARG, "nat_frames %d < 0", cfg->nat_frames);
    for (int i = 0; i < cfg->numlayers; i++)
        if (cfg->layersizes[i] < 1) return fail(MLGGD_ERR_ARG, "layersizes[%d] = %d", i, cfg->layersizes[i]);
    if (cfg->mask_bins < 0) return fail(MLGGD_ERR_ARG, "mask_bins %d < 0", cfg->mask_bins);
    if (cfg->mask_bins > 0 && (long long)cfg->layersizes[cfg->numlayers - 1] != 2ll * cfg->mask_bins)
        return fail(MLGGD_ERR_ARG, "mask_bins %d: the last layer must have 2 x %d units (LPS and mask), not %d",
                    cfg->mask_bins, cfg->mask_bins, cfg->layersizes[cfg->numlayers - 1]);
    for (int i = 1; i < cfg->numlayers; i++) {
        // the kernels address a weight matrix with 32-bit byte offsets into one buffer resource
        const long long bytes = 4ll * ceil32(cfg->layersizes[i - 1]) * ceil32(cfg->layersizes[i]);
        if (bytes >= (1ll << 31))
            return fail(MLGGD_ERR_ARG, "layer %d: %d x %d weights exceed the 2 GiB a kernel can address", i,
                        cfg->layersizes[i - 1], cfg->layersizes[i]);
    }
    if (ceil32(cfg->bunchsize) > 1152)  // LOSS_LDS_MAX: 32 columns x (1152 + 1) frames of the loss kernels' LDS tile
        return fail(MLGGD_ERR_ARG, "bunchsize %d too large for the loss kernel's LDS tile (max 1152)", cfg->bunchsize);
    int ndev = 0;
    hipError_t de = hipGetDeviceCount(&ndev);
    if (de != hipSuccess || ndev < 1)
        return fail(MLGGD_ERR_DEVICE, "no HIP device available (%s)", de == hipSuccess ? "count 0" : hipGetErrorString(de));
    // BP_GPU.cu:17-21 "GPU Num %d Not In Range"
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(MLGGD_ERR_ARG, "GPU Num %d Not In Range %d-%d", cfg->device, 0, ndev - 1);

    mlggd_engine *e = new mlggd_engine();
    e->cfg = *cfg;
    e->L = cfg->numlayers;
    e->device = cfg->device;
    for (int i = 0; i < e->L; i++) {
        e->ls[i] = cfg->layersizes[i];
        e->lsp[i] = ceil32(cfg->layersizes[i]);
    }
    e->B = cfg->bunchsize;
    e->Bp = ceil32(e->B);
    e->K0 = e->ls[0];
    e->D = e->ls[e->L - 1];
    e->Dp = e->lsp[e->L - 1];
    e->nat_frames = cfg->nat_frames;
    e->mask_bins = cfg->mask_bins;
    if (const char *v = getenv("MLGGD_WAVES_LOOKUP")) e->ww.lookup_table = !strcmp(v, "table");
    if (const char *v = getenv("MLGGD_DW_TILE")) e->dw_tile = atoi(v);
    if (const char *v = getenv("MLGGD_DW_PERSIST")) e->dw_persist = atoi(v);
    if (const char *v = getenv("MLGGD_DWP_PER_CU")) e->dwp_per_cu = atoi(v);
    if (const char *v = getenv("MLGGD_DW_MERGE")) e->dw_merge = atoi(v);
    if (const char *v = getenv("MLGGD_LOSS_FUSE")) e->loss_fuse = atoi(v);
    if (const char *v = getenv("MLGGD_TILE_MAP")) e->tile_map = atoi(v);
    if (const char *v = getenv("MLGGD_STAGE_AHEAD")) e->stage_ahead = atoi(v);
    if (const char *v = getenv("MLGGD_CV_DEVICE")) e->cv_device = atoi(v) ? 1 : 0;
    if (const char *v = getenv("MLGGD_TILE64")) e->tile64 = atoi(v);
    *out = e;  // so the caller can destroy on failure

    roctx_load();
    HIPCHK(hipSetDevice(e->device));
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device) == hipSuccess && cus > 0) e->n_cus = cus;
    }
    HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    // (one compute stream: every HIP stream takes one of the process's few hardware queues, and two streams of one engine
    // that land on the SAME queue serialise -- round 3: the first communicator engine created after other engines had
    // come and gone ran its step in 251 instead of 173 us because its communication stream shared a queue with its main
    // stream)
    HIPCHK(hipEventCreate(&e->ev_t0));
    HIPCHK(hipEventCreate(&e->ev_t1));

    const int L = e->L, Bp = e->Bp;
    CHK(dev_alloc(e, &e->Yt[0], (size_t)e->lsp[0] * Bp));
    CHK(dev_alloc(e, &e->in_bunch_buf[0], (size_t)(Bp + 1) * e->lsp[0]));
    CHK(dev_alloc(e, &e->in_bunch_buf[1], (size_t)(Bp + 1) * e->lsp[0]));
    e->in_bunch = e->in_bunch_buf[0];
    for (int l = 1; l < L; l++) {
        const size_t wsz = (size_t)e->lsp[l - 1] * e->lsp[l];
        CHK(dev_alloc(e, &e->W[l], wsz));
        CHK(dev_alloc(e, &e->dW[l], wsz));
        CHK(dev_alloc(e, &e->bias[l], e->lsp[l]));
        CHK(dev_alloc(e, &e->dbias[l], e->lsp[l]));
        const size_t asz = (size_t)e->lsp[l] * Bp;
        if (l != L - 1) {
            CHK(dev_alloc(e, &e->Yt[l], asz));
            CHK(dev_alloc(e, &e->Y[l], asz));
        }
        CHK(dev_alloc(e, &e->dEdXt[l], asz));
        CHK(dev_alloc(e, &e->dEdX[l], asz));
    }
    // output-layer GEMM: split K across workgroups so the small N still fills the chip
    {
        const int tiles = (e->Dp / 32) * (Bp / 32);
        const int pairs = e->lsp[L - 2] / 2;
        // one round of workgroups on the 256 CUs when that still splits K at least four ways (36 tiles: 7 x 36 = 252
        // workgroups; 8 x 36 = 288 left 32 of them for a second round: +1 us per step), else enough to fill the chip
        int S = 256 / tiles >= 4 ? 256 / tiles : (256 + tiles - 1) / tiles;
        if (S > pairs / 16) S = pairs / 16;  // >= 4 k-pairs per wave
        if (S < 1) S = 1;
        if (S > 32) S = 32;
        if (const char *v = getenv("MLGGD_S_OUT")) S = atoi(v) < 1 ? 1 : atoi(v) > 32 ? 32 : atoi(v);  // A/B knob
        e->S_out = S;
    }
    CHK(dev_alloc(e, &e->slab, (size_t)e->S_out * e->Dp * Bp));
    CHK(dev_alloc(e, &e->outT, (size_t)e->Dp * Bp));
    CHK(dev_alloc(e, &e->eT, (size_t)e->Dp * Bp));
    CHK(dev_alloc(e, &e->pT, (size_t)e->Dp * Bp));
    CHK(dev_alloc(e, &e->colsum, e->Dp));
    CHK(dev_alloc(e, &e->scalefactor, e->Dp));

    const int rc = mlggd_set_weights(e, weights, bias);
    if (rc != MLGGD_OK) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}

int mlggd_destroy(mlggd_handle e) {
    if (!e) return MLGGD_OK;
    if (e->live_groups > 0)
        return fail(MLGGD_ERR_STATE, "%d live group(s) of this engine are open: mlggd_live_close them first",
                    e->live_groups);
    if (e->rbm_open > 0) return fail(MLGGD_ERR_STATE, "an RBM session of this engine is open: mlggd_rbm_close it first");
    hipSetDevice(e->device);
    if (e->stream) hipStreamSynchronize(e->stream);
    if (e->comm_stream) hipStreamSynchronize(e->comm_stream);
    if (e->stat_comm && g_rccl.CommDestroy) g_rccl.CommDestroy(e->stat_comm);
    if (e->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(e->comm);
    for (void *p : e->allocs) hipFree(p);
    if (e->copy_stream) hipStreamSynchronize(e->copy_stream);
    for (auto &r : e->raw)
        if (r.last_use) hipEventDestroy(r.last_use);
    if (e->copy_stream) hipStreamDestroy(e->copy_stream);
    for (hipEvent_t ev : e->prof_ev) hipEventDestroy(ev);
    for (int l = 0; l < MLGGD_MAXLAYER; l++) {
        if (e->ev_grad[l]) hipEventDestroy(e->ev_grad[l]);
        if (e->ev_red[l]) hipEventDestroy(e->ev_red[l]);
    }
    for (int l = 0; l < MLGGD_MAXLAYER; l++) {
        if (e->ev_W[l]) hipEventDestroy(e->ev_W[l]);
        if (e->ev_layer[l]) hipEventDestroy(e->ev_layer[l]);
    }
    if (e->ev_dw_done) hipEventDestroy(e->ev_dw_done);
    if (e->ev_ready) hipEventDestroy(e->ev_ready);
    if (e->ev_gathered) hipEventDestroy(e->ev_gathered);
    if (e->ev_bias) hipEventDestroy(e->ev_bias);
    if (e->ev_bias_red) hipEventDestroy(e->ev_bias_red);
    if (e->ev_t0) hipEventDestroy(e->ev_t0);
    if (e->ev_t1) hipEventDestroy(e->ev_t1);
    if (e->comm_stream) hipStreamDestroy(e->comm_stream);
    if (e->stream) hipStreamDestroy(e->stream);
    delete e;  // every DevBuf frees itself here: all streams have been synchronised above
    return MLGGD_OK;
}

int mlggd_set_weights(mlggd_handle e, const float *const *weights, const float *const *bias) {
    if (!e || !weights || !bias) return fail(MLGGD_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(e->device));
    for (int l = 1; l < e->L; l++)  // before the first upload: a rejected call leaves every layer as it was
        if (!weights[l] || !bias[l]) return fail(MLGGD_ERR_ARG, "weights[%d] or bias[%d] is NULL", l, l);
    CHK(wait_weight_gathers(e, 1, e->L - 1));
    for (int l = 1; l < e->L; l++) {
        CHK(upload_padded(e->W[l], e->lsp[l], weights[l], e->ls[l - 1], e->ls[l], e->stream));  // BP_GPU.cu:106
        HIPCHK(hipMemcpyAsync(e->bias[l], bias[l], (size_t)e->ls[l] * 4, hipMemcpyHostToDevice, e->stream));  // :107
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}

int mlggd_get_weights(mlggd_handle e, float *const *weights, float *const *bias) {
    if (!e || !weights || !bias) return fail(MLGGD_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(e->device));
    CHK(wait_weight_gathers(e, 1, e->L - 1));
    for (int l = 1; l < e->L; l++) {
        if (!weights[l] || !bias[l]) return fail(MLGGD_ERR_ARG, "weights[%d] or bias[%d] is NULL", l, l);
        CHK(download_padded(weights[l], e->W[l], e->lsp[l], e->ls[l - 1], e->ls[l], e->stream));  // BP_GPU.cu:522
        HIPCHK(hipMemcpyAsync(bias[l], e->bias[l], (size_t)e->ls[l] * 4, hipMemcpyDeviceToHost, e->stream));  // :523
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}

int mlggd_get_scalefactor(mlggd_handle e, float *alpha) {
    if (!e || !alpha) return fail(MLGGD_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(alpha, e->scalefactor, (size_t)e->D * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}

// the learned scale's state: where alpha / v of the copy the NEXT step reads live
static float *scale_alpha_cur(mlggd_engine *e) { return e->scale_state.p + scale_rule::alpha_at(e->scale_cur, (size_t)e->Dp, 0); }
static float *scale_velocity_cur(mlggd_engine *e) { return e->scale_state.p + scale_rule::velocity_at(e->scale_cur, (size_t)e->Dp, 0); }
static int scale_check_alpha(const mlggd_engine *e, const float *alpha) {
    for (int d = 0; d < e->D; d++)
        if (!scale_rule::valid_alpha(alpha[d]))
            return fail(MLGGD_ERR_ARG, "alpha[%d] = %g: a scale must be finite and not negative (0: the bin seeds from its "
                        "first minibatch)", d, (double)alpha[d]);
    return MLGGD_OK;
}

int mlggd_set_scalefactor(mlggd_handle e, const float *alpha) {
    if (!e || !alpha) return fail(MLGGD_ERR_ARG, "NULL argument");
    const bool learned = e->scale_mode == MLGGD_SCALE_LEARNED;  // alpha is then the state's: set it there too, v stays
    if (learned) CHK(scale_check_alpha(e, alpha));
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->scalefactor, alpha, (size_t)e->D * 4, hipMemcpyHostToDevice, e->stream));
    if (learned) HIPCHK(hipMemcpyAsync(scale_alpha_cur(e), alpha, (size_t)e->D * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}

// ------------------------------------------------------------------ learned scale per output bin (scale_rule.h)
int mlggd_set_scale_mode(mlggd_handle e, int mode, float lrate, float momentum, float vmax) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (e->cfg.MLflag != 1)
        return fail(MLGGD_ERR_STATE, "a scale mode needs the ML-GGD loss (MLflag 1), this engine has MLflag %d: a beta-norm "
                    "has no scale", e->cfg.MLflag);
    if (mode != MLGGD_SCALE_ALTERNATING && mode != MLGGD_SCALE_LEARNED)
        return fail(MLGGD_ERR_ARG, "scale mode %d: must be %d (alternating) or %d (learned)", mode, MLGGD_SCALE_ALTERNATING,
                    MLGGD_SCALE_LEARNED);
    if (!scale_rule::valid(mode, lrate, momentum, vmax))
        return fail(MLGGD_ERR_ARG, "scale lrate %g, momentum %g, vmax %g: finite values with lrate >= 0, 0 <= momentum < 1 "
                    "and vmax > 0 are required", (double)lrate, (double)momentum, (double)vmax);
    if (mode == MLGGD_SCALE_LEARNED && e->scale_mode != MLGGD_SCALE_LEARNED) {
        HIPCHK(hipSetDevice(e->device));
        const size_t n = devbuf_rule::scale_state_floats((size_t)e->Dp);
        HIPCHK(e->scale_state.grow(n, n, e->bufs, nullptr, nullptr));
        // on the engine's stream: behind every step already enqueued, which may still write scalefactor
        HIPCHK(hipMemsetAsync(e->scale_state.p, 0, n * sizeof(float), e->stream));
        e->scale_cur = 0;
        HIPCHK(hipMemcpyAsync(scale_alpha_cur(e), e->scalefactor, (size_t)e->D * 4, hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        e->scale_steps = 0;
    }
    // kernel arguments of the launches to come: steps already enqueued chose their kernels when they were enqueued
    e->scale_mode = mode, e->scale_lrate = lrate, e->scale_momentum = momentum, e->scale_vmax = vmax;
    return MLGGD_OK;
}

int mlggd_get_scale_mode(mlggd_handle e, int *mode, float *lrate, float *momentum, float *vmax, int64_t *steps) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (mode) *mode = e->scale_mode;
    if (lrate) *lrate = e->scale_lrate;
    if (momentum) *momentum = e->scale_momentum;
    if (vmax) *vmax = e->scale_vmax;
    if (steps) *steps = (int64_t)e->scale_steps;
    return MLGGD_OK;
}

int mlggd_get_scale_state(mlggd_handle e, float *alpha, float *velocity) {
    if (!e || !alpha) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (e->scale_mode != MLGGD_SCALE_LEARNED) return fail(MLGGD_ERR_STATE, "mlggd_get_scale_state: the scale mode is not learned");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(alpha, scale_alpha_cur(e), (size_t)e->D * 4, hipMemcpyDeviceToHost, e->stream));
    if (velocity) HIPCHK(hipMemcpyAsync(velocity, scale_velocity_cur(e), (size_t)e->D * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}

int mlggd_set_scale_state(mlggd_handle e, const float *alpha, const float *velocity) {
    if (!e || !alpha) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (e->scale_mode != MLGGD_SCALE_LEARNED) return fail(MLGGD_ERR_STATE, "mlggd_set_scale_state: the scale mode is not learned");
    CHK(scale_check_alpha(e, alpha));
    if (velocity)
        for (int d = 0; d < e->D; d++)
            if (!std::isfinite(velocity[d]))
                return fail(MLGGD_ERR_ARG, "velocity[%d] = %g: a velocity must be finite", d, (double)velocity[d]);
    HIPCHK(hipSetDevice(e->device));
    const std::vector<float> zeros(velocity ? 0 : e->D, 0.0f);
    // on the engine's stream: behind every step already enqueued, which may still write this copy
    HIPCHK(hipMemcpyAsync(scale_alpha_cur(e), alpha, (size_t)e->D * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(scale_velocity_cur(e), velocity ? velocity : zeros.data(), (size_t)e->D * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->scalefactor, alpha, (size_t)e->D * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}

int mlggd_read_scale_state(const char *path, int D, float *alpha, float *velocity) {
    if (!path || !alpha) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (D < 1) return fail(MLGGD_ERR_ARG, "D %d < 1", D);
    std::string err;
    if (!mlggd_host::parse_scale_state(path, D, alpha, velocity, &err)) return fail(MLGGD_ERR_ARG, "%s", err.c_str());
    return MLGGD_OK;
}

int mlggd_write_scale_state(const char *path, int D, const float *alpha, const float *velocity, float lrate, float momentum,
                            float vmax, int64_t steps) {
    if (!path || !alpha) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (D < 1) return fail(MLGGD_ERR_ARG, "D %d < 1", D);
    std::string err;
    const mlggd_host::ScaleFileHeader h = {lrate, momentum, vmax, (long long)steps};
    if (!mlggd_host::write_scale_state(path, D, alpha, velocity, h, &err)) return fail(MLGGD_ERR_ARG, "%s", err.c_str());
    return MLGGD_OK;
}

// ------------------------------------------------------------------ Adam beside SGD with momentum (adam_rule.h)
// the mode's buffers, allocated on first entry; the moments zeroed on the engine's stream, behind every step enqueued
static int adam_enter(mlggd_engine *e) {
    HIPCHK(hipSetDevice(e->device));
    if (!e->adam_gb.p) {
        size_t gbn = 0;
        for (int l = 1; l < e->L; l++) gbn += e->lsp[l];
        HIPCHK(e->adam_gb.grow(gbn, gbn, e->bufs, &e->stream, nullptr));
        e->gb_all = e->adam_gb.p;
        e->gb_all_count = gbn;
        size_t off = 0;
        for (int l = e->L - 1; l >= 1; l--) {
            e->gb[l] = e->gb_all + off;
            off += e->lsp[l];
        }
    }
    for (int l = 1; l < e->L; l++) {
        const size_t n = (size_t)e->lsp[l - 1] * e->lsp[l], nb = (size_t)e->lsp[l];
        if (!e->adam_G[l].p) {  // pads are zero from here on: the dW launches write the real rows and columns only
            HIPCHK(e->adam_G[l].grow(n, n, e->bufs, &e->stream, nullptr));
            e->G[l] = e->adam_G[l].p;
        }
        HIPCHK(e->adam_mw[l].grow(n, n, e->bufs, nullptr, nullptr));
        HIPCHK(e->adam_vw[l].grow(n, n, e->bufs, nullptr, nullptr));
        HIPCHK(e->adam_mb[l].grow(nb, nb, e->bufs, nullptr, nullptr));
        HIPCHK(e->adam_vb[l].grow(nb, nb, e->bufs, nullptr, nullptr));
        HIPCHK(hipMemsetAsync(e->adam_mw[l].p, 0, n * sizeof(float), e->stream));
        HIPCHK(hipMemsetAsync(e->adam_vw[l].p, 0, n * sizeof(float), e->stream));
        HIPCHK(hipMemsetAsync(e->adam_mb[l].p, 0, nb * sizeof(float), e->stream));
        HIPCHK(hipMemsetAsync(e->adam_vb[l].p, 0, nb * sizeof(float), e->stream));
    }
    return MLGGD_OK;
}

int mlggd_set_optimizer(mlggd_handle e, int kind, float beta1, float beta2, float eps) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (!adam_rule::valid_kind(kind))
        return fail(MLGGD_ERR_ARG, "optimizer %d: must be %d (SGD with momentum) or %d (Adam)", kind, MLGGD_OPT_SGD, MLGGD_OPT_ADAM);
    if (!adam_rule::valid(beta1, beta2, eps))
        return fail(MLGGD_ERR_ARG, "beta1 %g, beta2 %g, eps %g: betas in [0, 1) and a finite eps > 0 are required", (double)beta1,
                    (double)beta2, (double)eps);
    if (kind == MLGGD_OPT_ADAM) {
        if (e->comm || e->fake_world)
            return fail(MLGGD_ERR_STATE, "mlggd_set_optimizer: Adam runs on a single-device engine, this one has joined a "
                        "communicator or an emulated world");
        CHK(adam_enter(e));
        e->adam_b1 = beta1, e->adam_b2 = beta2, e->adam_eps = eps;
        e->adam_steps = 0;
        e->adam_prod = adam_rule::Products();
    }
    // the launches to come: steps already enqueued chose their kernels when they were enqueued.  The SGD momentum
    // buffers are touched in neither direction.
    e->opt_kind = kind;
    return MLGGD_OK;
}

int mlggd_get_optimizer(mlggd_handle e, int *kind, float *beta1, float *beta2, float *eps, int64_t *steps) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (kind) *kind = e->opt_kind;
    if (beta1) *beta1 = e->adam_b1;
    if (beta2) *beta2 = e->adam_b2;
    if (eps) *eps = e->adam_eps;
    if (steps) *steps = (int64_t)e->adam_steps;
    return MLGGD_OK;
}

int mlggd_get_optimizer_state(mlggd_handle e, float *const *m_w, float *const *v_w, float *const *m_b, float *const *v_b) {
    if (!e || !m_w || !v_w || !m_b || !v_b) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (e->opt_kind != MLGGD_OPT_ADAM) return fail(MLGGD_ERR_STATE, "mlggd_get_optimizer_state: the optimizer is not Adam");
    for (int l = 1; l < e->L; l++)
        if (!m_w[l] || !v_w[l] || !m_b[l] || !v_b[l]) return fail(MLGGD_ERR_ARG, "a moment array of layer %d is NULL", l);
    HIPCHK(hipSetDevice(e->device));
    for (int l = 1; l < e->L; l++) {
        CHK(download_padded(m_w[l], e->adam_mw[l].p, e->lsp[l], e->ls[l - 1], e->ls[l], e->stream));
        CHK(download_padded(v_w[l], e->adam_vw[l].p, e->lsp[l], e->ls[l - 1], e->ls[l], e->stream));
        HIPCHK(hipMemcpyAsync(m_b[l], e->adam_mb[l].p, (size_t)e->ls[l] * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(v_b[l], e->adam_vb[l].p, (size_t)e->ls[l] * 4, hipMemcpyDeviceToHost, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}

int mlggd_set_optimizer_state(mlggd_handle e, const float *const *m_w, const float *const *v_w, const float *const *m_b,
                              const float *const *v_b, int64_t steps) {
    if (!e || !m_w || !v_w || !m_b || !v_b) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (e->opt_kind != MLGGD_OPT_ADAM) return fail(MLGGD_ERR_STATE, "mlggd_set_optimizer_state: the optimizer is not Adam");
    if (steps < 0) return fail(MLGGD_ERR_ARG, "steps %lld < 0", (long long)steps);
    for (int l = 1; l < e->L; l++) {
        if (!m_w[l] || !v_w[l] || !m_b[l] || !v_b[l]) return fail(MLGGD_ERR_ARG, "a moment array of layer %d is NULL", l);
        const size_t n = (size_t)e->ls[l - 1] * e->ls[l], nb = (size_t)e->ls[l];
        for (size_t i = 0; i < n + nb; i++) {
            const float m = i < n ? m_w[l][i] : m_b[l][i - n], v = i < n ? v_w[l][i] : v_b[l][i - n];
            if (!std::isfinite(m) || !std::isfinite(v) || v < 0.0f)
                return fail(MLGGD_ERR_ARG, "layer %d, %s %zu: m = %g, v = %g -- a first moment must be finite, a second moment "
                            "finite and not negative", l, i < n ? "weight" : "bias", i < n ? i : i - n, (double)m, (double)v);
        }
    }
    HIPCHK(hipSetDevice(e->device));
    // on the engine's stream: behind every step already enqueued.  The pads of the device arrays are not touched.
    for (int l = 1; l < e->L; l++) {
        CHK(upload_padded(e->adam_mw[l].p, e->lsp[l], m_w[l], e->ls[l - 1], e->ls[l], e->stream));
        CHK(upload_padded(e->adam_vw[l].p, e->lsp[l], v_w[l], e->ls[l - 1], e->ls[l], e->stream));
        HIPCHK(hipMemcpyAsync(e->adam_mb[l].p, m_b[l], (size_t)e->ls[l] * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->adam_vb[l].p, v_b[l], (size_t)e->ls[l] * 4, hipMemcpyHostToDevice, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    e->adam_steps = (long long)steps;
    e->adam_prod = adam_rule::products(e->adam_b1, e->adam_b2, steps);
    return MLGGD_OK;
}

int mlggd_adam_apply(float *w, float *m, float *v, const float *G, int64_t n, float nf, float weightcost, float lrate, float beta1,
                     float beta2, float eps, int64_t steps_before) {
    if (n < 0 || steps_before < 0) return fail(MLGGD_ERR_ARG, "n %lld or steps_before %lld < 0", (long long)n, (long long)steps_before);
    if (n > 0 && (!w || !m || !v || !G)) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (!adam_rule::valid(beta1, beta2, eps))
        return fail(MLGGD_ERR_ARG, "beta1 %g, beta2 %g, eps %g: betas in [0, 1) and a finite eps > 0 are required", (double)beta1,
                    (double)beta2, (double)eps);
    const int64_t t = steps_before == INT64_MAX ? INT64_MAX : steps_before + 1;  // the products are spent long before
    const adam_rule::Consts c = adam_rule::consts(nf, lrate, beta1, beta2, eps, adam_rule::products(beta1, beta2, t));
    for (int64_t i = 0; i < n; i++) {
        const adam_rule::Moments r = adam_rule::step(w[i], m[i], v[i], G[i], weightcost, c);
        w[i] = r.w, m[i] = r.m, v[i] = r.v;
    }
    return MLGGD_OK;
}

int mlggd_write_optimizer_state(const char *path, int numlayers, const int32_t *layersizes, const float *const *m_w,
                                const float *const *v_w, const float *const *m_b, const float *const *v_b, float beta1, float beta2,
                                float eps, int64_t steps) {
    if (!path || (numlayers > 0 && !layersizes) || (numlayers > 1 && (!m_w || !v_w || !m_b || !v_b)))
        return fail(MLGGD_ERR_ARG, "NULL argument");
    if (!adam_rule::valid(beta1, beta2, eps))
        return fail(MLGGD_ERR_ARG, "beta1 %g, beta2 %g, eps %g: betas in [0, 1) and a finite eps > 0 are required", (double)beta1,
                    (double)beta2, (double)eps);
    for (int l = 1; l < numlayers; l++)
        if (!m_w[l] || !v_w[l] || !m_b[l] || !v_b[l]) return fail(MLGGD_ERR_ARG, "a moment array of layer %d is NULL", l);
    std::string err;
    const std::vector<int> ls(layersizes, layersizes + (numlayers > 0 ? numlayers : 0));
    if (!mlggd_host::write_opt_state(path, numlayers, ls.data(), beta1, beta2, eps, (long long)steps, m_w, v_w, m_b, v_b, &err))
        return fail(MLGGD_ERR_ARG, "%s", err.c_str());
    return MLGGD_OK;
}

int mlggd_read_optimizer_header(const char *path, int32_t *numlayers, int32_t *layersizes, float *beta1, float *beta2, float *eps,
                                int64_t *steps) {
    if (!path || !numlayers || !layersizes) return fail(MLGGD_ERR_ARG, "NULL argument");
    mlggd_host::OptState s;
    std::string err;
    if (!mlggd_host::read_opt_header(path, &s, &err)) return fail(MLGGD_ERR_ARG, "%s", err.c_str());
    if (s.layersizes.size() > (size_t)MLGGD_MAXLAYER)
        return fail(MLGGD_ERR_ARG, "%s: %zu layers, an engine has at most %d", path, s.layersizes.size(), MLGGD_MAXLAYER);
    *numlayers = (int32_t)s.layersizes.size();
    for (size_t l = 0; l < s.layersizes.size(); l++) layersizes[l] = s.layersizes[l];
    if (beta1) *beta1 = s.beta1;
    if (beta2) *beta2 = s.beta2;
    if (eps) *eps = s.eps;
    if (steps) *steps = (int64_t)s.steps;
    return MLGGD_OK;
}

int mlggd_read_optimizer_state(const char *path, int numlayers, const int32_t *layersizes, float *const *m_w, float *const *v_w,
                               float *const *m_b, float *const *v_b, float *beta1, float *beta2, float *eps, int64_t *steps) {
    if (!path || numlayers < 0 || (numlayers > 0 && !layersizes) || (numlayers > 1 && (!m_w || !v_w || !m_b || !v_b)))
        return fail(MLGGD_ERR_ARG, "NULL argument");
    for (int l = 1; l < numlayers; l++)
        if (!m_w[l] || !v_w[l] || !m_b[l] || !v_b[l]) return fail(MLGGD_ERR_ARG, "a moment array of layer %d is NULL", l);
    mlggd_host::OptState s;
    std::string err;
    const std::vector<int> ls(layersizes, layersizes + numlayers);
    if (!mlggd_host::read_opt_state(path, ls.data(), numlayers, &s, &err)) return fail(MLGGD_ERR_ARG, "%s", err.c_str());
    for (int l = 1; l < numlayers; l++) {
        memcpy(m_w[l], s.m_w[l - 1].data(), s.m_w[l - 1].size() * sizeof(float));
        memcpy(v_w[l], s.v_w[l - 1].data(), s.v_w[l - 1].size() * sizeof(float));
        memcpy(m_b[l], s.m_b[l - 1].data(), s.m_b[l - 1].size() * sizeof(float));
        memcpy(v_b[l], s.v_b[l - 1].data(), s.v_b[l - 1].size() * sizeof(float));
    }
    if (beta1) *beta1 = s.beta1;
    if (beta2) *beta2 = s.beta2;
    if (eps) *eps = s.eps;
    if (steps) *steps = (int64_t)s.steps;
    return MLGGD_OK;
}

int mlggd_set_shapefactors(mlggd_handle e, const float *betas) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (!betas) {  // steps already enqueued chose their kernels when they were enqueued
        e->per_bin = false;
        e->betas_host.clear();
        return MLGGD_OK;
    }
    if (e->cfg.MLflag != 1)
        return fail(MLGGD_ERR_STATE, "per-bin shape factors need the ML-GGD loss (MLflag 1), this engine has MLflag %d: a "
                    "beta-norm whose exponent differs per bin has no per-bin scale", e->cfg.MLflag);
    for (int d = 0; d < e->D; d++)
        if (!(betas[d] > 0.0f) || !std::isfinite(betas[d]))
            return fail(MLGGD_ERR_ARG, "betas[%d] = %g: a shape must be positive and finite", d, (double)betas[d]);
    HIPCHK(hipSetDevice(e->device));
    if (!e->betas_dev) CHK(dev_alloc(e, &e->betas_dev, e->Dp));
    std::vector<float> padded(e->Dp, 1.0f);
    std::copy(betas, betas + e->D, padded.begin());
    // on the engine's stream: behind every step already enqueued, which may still read the previous vector
    HIPCHK(hipMemcpyAsync(e->betas_dev, padded.data(), (size_t)e->Dp * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->betas_host.assign(betas, betas + e->D);
    e->per_bin = true;
    return MLGGD_OK;
}

int mlggd_get_shapefactors(mlggd_handle e, float *betas) {
    if (!e || !betas) return fail(MLGGD_ERR_ARG, "NULL argument");
    for (int d = 0; d < e->D; d++) betas[d] = e->per_bin ? e->betas_host[d] : e->cfg.shapefactor;
    return MLGGD_OK;
}

int mlggd_read_shapefactors(const char *path, int D, float fallback, float *betas) {
    if (!path || !betas) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (D < 1) return fail(MLGGD_ERR_ARG, "D %d < 1", D);
    std::string err;
    if (!mlggd_host::parse_shapefactors(path, D, fallback, betas, &err)) return fail(MLGGD_ERR_ARG, "%s", err.c_str());
    return MLGGD_OK;
}

// ------------------------------------------------------------------ asymmetric error model (asym_rule.h)
int mlggd_set_asymmetry(mlggd_handle e, const float *kappas) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (!kappas) {  // steps already enqueued chose their kernels when they were enqueued
        e->asym = false;
        e->kappas_host.clear();
        return MLGGD_OK;
    }
    if (e->cfg.MLflag != 1)
        return fail(MLGGD_ERR_STATE, "a skew per bin needs the ML-GGD loss (MLflag 1), this engine has MLflag %d: a "
                    "beta-norm has no density to skew", e->cfg.MLflag);
    for (int d = 0; d < e->D; d++)
        if (!(kappas[d] > 0.0f) || !std::isfinite(kappas[d]))
            return fail(MLGGD_ERR_ARG, "kappas[%d] = %g: a skew must be positive and finite", d, (double)kappas[d]);
    HIPCHK(hipSetDevice(e->device));
    const size_t Dp = (size_t)e->Dp;
    const bool first = !e->asym_betas_dev.p;
    HIPCHK(e->kappas_dev.grow(Dp, Dp, e->bufs, nullptr, nullptr));
    HIPCHK(e->asym_betas_dev.grow(Dp, Dp, e->bufs, nullptr, nullptr));
    std::vector<float> padded(Dp, 1.0f), shapes(Dp, 1.0f);
    std::copy(kappas, kappas + e->D, padded.begin());
    std::fill(shapes.begin(), shapes.begin() + e->D, e->cfg.shapefactor);
    // on the engine's stream: behind every step already enqueued, which may still read the previous vector
    HIPCHK(hipMemcpyAsync(e->kappas_dev.p, padded.data(), Dp * 4, hipMemcpyHostToDevice, e->stream));
    if (first) HIPCHK(hipMemcpyAsync(e->asym_betas_dev.p, shapes.data(), Dp * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->kappas_host.assign(kappas, kappas + e->D);
    e->asym = true;
    return MLGGD_OK;
}

int mlggd_get_asymmetry(mlggd_handle e, float *kappas) {
    if (!e || !kappas) return fail(MLGGD_ERR_ARG, "NULL argument");
    for (int d = 0; d < e->D; d++) kappas[d] = e->asym ? e->kappas_host[d] : 1.0f;
    return MLGGD_OK;
}

int mlggd_read_asymmetry(const char *path, int D, float fallback, float *kappas) {
    if (!path || !kappas) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (D < 1) return fail(MLGGD_ERR_ARG, "D %d < 1", D);
    std::string err;
    if (!mlggd_host::parse_asymmetry(path, D, fallback, kappas, &err)) return fail(MLGGD_ERR_ARG, "%s", err.c_str());
    return MLGGD_OK;
}

// ------------------------------------------------------------------ global variance equalisation (gv_rule.h)
int mlggd_set_gv(mlggd_handle e, const float *eta) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (!eta) {  // decode calls already made have enqueued their launches with the factors they saw
        e->gv_on = false;
        e->gv_host.clear();
        return MLGGD_OK;
    }
    for (int d = 0; d < e->D; d++)
        if (!(eta[d] > 0.0f) || !std::isfinite(eta[d]))
            return fail(MLGGD_ERR_ARG, "eta[%d] = %g: a factor must be positive and finite", d, (double)eta[d]);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(e->gv_dev.grow((size_t)e->D, (size_t)e->D, e->bufs, nullptr, nullptr));
    // on the engine's stream: behind every decode already enqueued, which may still read the previous vector
    HIPCHK(hipMemcpyAsync(e->gv_dev.p, eta, (size_t)e->D * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->gv_host.assign(eta, eta + e->D);
    e->gv_on = true;
    return MLGGD_OK;
}

int mlggd_get_gv(mlggd_handle e, float *eta) {
    if (!e || !eta) return fail(MLGGD_ERR_ARG, "NULL argument");
    for (int d = 0; d < e->D; d++) eta[d] = e->gv_on ? e->gv_host[d] : 1.0f;
    return MLGGD_OK;
}

// ------------------------------------------------------------------ mask post-filter (mask_rule.h)
int mlggd_set_mask(mlggd_handle e, int mode, float lo, float hi, float scale) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (!e->mask_bins) return fail(MLGGD_ERR_STATE, "mlggd_set_mask: the engine was created without mask_bins");
    if (mode != MLGGD_MASK_OFF && mode != MLGGD_MASK_SELECT)
        return fail(MLGGD_ERR_ARG, "mask mode %d: must be %d (off) or %d (select)", mode, MLGGD_MASK_OFF, MLGGD_MASK_SELECT);
    if (!mask_rule::valid(mode, lo, hi, scale))
        return fail(MLGGD_ERR_ARG, "mask lo %g, hi %g, scale %g: finite values with lo <= hi and scale > 0 are required",
                    (double)lo, (double)hi, (double)scale);
    // kernel arguments of the launches to come: those already enqueued carry the values they were launched with
    e->mask_mode = mode, e->mask_lo = lo, e->mask_hi = hi, e->mask_scale = scale;
    return MLGGD_OK;
}

int mlggd_get_mask(mlggd_handle e, int *mode, float *lo, float *hi, float *scale) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (!e->mask_bins) return fail(MLGGD_ERR_STATE, "mlggd_get_mask: the engine was created without mask_bins");
    if (mode) *mode = e->mask_mode;
    if (lo) *lo = e->mask_lo;
    if (hi) *hi = e->mask_hi;
    if (scale) *scale = e->mask_scale;
    return MLGGD_OK;
}

int mlggd_get_mask_bins(mlggd_handle e, int *mask_bins) {
    if (!e || !mask_bins) return fail(MLGGD_ERR_ARG, "NULL argument");
    *mask_bins = e->mask_bins;
    return MLGGD_OK;
}

// Host only, no device: the post-filter on given rows, straight from the header.
int mlggd_mask_select(int D, int64_t n, const float *noisy_lps, const float *lps, const float *mask, float lo, float hi,
                      float *out) {
    if (D < 1) return fail(MLGGD_ERR_ARG, "D %d < 1", D);
    if (n < 0) return fail(MLGGD_ERR_ARG, "n %lld < 0", (long long)n);
    if (!mask_rule::valid(mask_rule::kSelect, lo, hi, 1.0f))
        return fail(MLGGD_ERR_ARG, "mask lo %g, hi %g: finite values with lo <= hi are required", (double)lo, (double)hi);
    if (n == 0) return MLGGD_OK;
    if (!noisy_lps || !lps || !mask || !out) return fail(MLGGD_ERR_ARG, "noisy_lps/lps/mask/out is NULL");
    mask_rule::select_rows(D, (size_t)n, noisy_lps, lps, mask, lo, hi, out);
    return MLGGD_OK;
}

int mlggd_read_gv(const char *path, int D, int shared, float *eta) {
    if (!path || !eta) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (D < 1) return fail(MLGGD_ERR_ARG, "D %d < 1", D);
    std::string err;
    if (!mlggd_host::parse_gv(path, D, shared != 0, eta, &err)) return fail(MLGGD_ERR_ARG, "%s", err.c_str());
    return MLGGD_OK;
}

// Host only, no device: the per-bin and the shared factor from the sums of mlggd_output_stats.
int mlggd_gv_fit(int D, int64_t n, const double *sums, double *gv_est, double *gv_ref, float *eta, uint8_t *fitted,
                 double *gv_est_shared, double *gv_ref_shared, float *eta_shared, int32_t *fitted_shared) {
    if (D < 1) return fail(MLGGD_ERR_ARG, "D %d < 1", D);
    if (n <= 0) return fail(MLGGD_ERR_ARG, "n %lld: the fit needs at least one sample", (long long)n);
    if (!sums) return fail(MLGGD_ERR_ARG, "sums is NULL");
    const gv_rule::Fit s = gv_rule::fit_all(D, n, sums, gv_est, gv_ref, eta, fitted);
    if (gv_est_shared) *gv_est_shared = s.gv_est;
    if (gv_ref_shared) *gv_ref_shared = s.gv_ref;
    if (eta_shared) *eta_shared = s.eta;
    if (fitted_shared) *fitted_shared = s.fitted ? 1 : 0;
    return MLGGD_OK;
}

int mlggd_set_cv_device_reduce(mlggd_handle e, int on) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    e->cv_device = on ? 1 : 0;
    return MLGGD_OK;
}

int mlggd_set_lrate(mlggd_handle e, float lrate) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    e->cfg.lrate = lrate;
    return MLGGD_OK;
}

static int ensure_chunk(mlggd_engine *e, int n_frames) {
    const size_t need = devbuf_rule::sample_slots((size_t)n_frames, (size_t)e->Bp);  // rows
    HIPCHK(e->chunk_in.grow(need * e->K0, need * e->K0, e->bufs, &e->stream, nullptr));
    HIPCHK(e->chunk_targ.grow(need * e->D, need * e->D, e->bufs, &e->stream, nullptr));
    return MLGGD_OK;
}

// the most samples one chunk may hold
static int chunk_cap(const mlggd_engine *e) {
    return e->cfg.max_cache_frames > 0 ? e->cfg.max_cache_frames : MLGGD_MAXCACHEFRAME;
}

static int check_frames(mlggd_engine *e, int n_frames) {
    if (n_frames < 0) return fail(MLGGD_ERR_ARG, "n_frames %d < 0", n_frames);
    const int cap = chunk_cap(e);
    if (n_frames > cap) return fail(MLGGD_ERR_ARG, "n_frames %d exceeds the chunk capacity %d", n_frames, cap);
    return MLGGD_OK;
}

int mlggd_load_chunk(mlggd_handle e, int n_frames, const float *in, const float *targ) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    CHK(check_frames(e, n_frames));
    if (n_frames > 0 && !in) return fail(MLGGD_ERR_ARG, "in is NULL");
    HIPCHK(hipSetDevice(e->device));
    CHK(ensure_chunk(e, n_frames));
    // todev_vf_vf("in"/"targ"), BP_GPU.cu:163-164
    if (n_frames > 0) {
        HIPCHK(hipMemcpyAsync(e->chunk_in.p, in, (size_t)n_frames * e->K0 * 4, hipMemcpyHostToDevice, e->stream));
        if (targ)
            HIPCHK(hipMemcpyAsync(e->chunk_targ.p, targ, (size_t)n_frames * e->D * 4, hipMemcpyHostToDevice, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    e->chunk_frames = n_frames;
    e->indexed = false;
    return MLGGD_OK;
}

}  // extern "C"

// width of a stream row: layersizes[0] / fea_context, or / (fea_context + 1) on a NAT engine (0: it does not divide)
static int stream_fdim(const mlggd_engine *e, int ctx) { return nat_rule::stream_width(e->K0, ctx, e->nat_frames > 0); }

// The engine's idle raw buffer set, grown (devbuf_rule.h) for a stream of `rows` rows read through windows of ctx rows,
// n samples and, on a NAT engine, n_nat noise rows; raw_set_commit then makes it the current one.  upload: the caller
// fills the set from host memory on copy_stream (mlggd_load_frames), else with kernels on the main stream; a fresh
// allocation is zero-filled on that stream.  The set's last reader (two chunks ago) has finished or is about to: it is
// waited for on the host before the allocation is touched.  A buffer that regrows drains the main stream first.
static int raw_set_acquire(mlggd_engine *e, int rows, int n, int ctx, int n_nat, bool upload, mlggd_engine::RawSet **out) {
    if (!e->copy_stream) {
        CHK(create_concurrent_stream(e, &e->copy_stream, "upload"));  // must not queue behind the chunk's kernels
        for (auto &r : e->raw) HIPCHK(hipEventCreateWithFlags(&r.last_use, hipEventDisableTiming));
    }
    const hipStream_t *zero = upload ? &e->copy_stream : &e->stream, *drain = &e->stream;
    const size_t fdim = (size_t)stream_fdim(e, ctx);
    mlggd_engine::RawSet &r = e->raw[e->raw_cur ^ 1];
    HIPCHK(hipEventSynchronize(r.last_use));
    const size_t n_feat = devbuf_rule::raw_feat_floats((size_t)rows, (size_t)ctx, fdim);
    const size_t n_targ = devbuf_rule::raw_rows((size_t)rows, (size_t)ctx) * e->D;
    const size_t n_slots = devbuf_rule::sample_slots((size_t)n, (size_t)e->Bp);
    HIPCHK(r.feat.grow(n_feat, n_feat, e->bufs, zero, drain));
    HIPCHK(r.targ.grow(n_targ, n_targ, e->bufs, zero, drain));
    HIPCHK(r.first.grow(n_slots, n_slots, e->bufs, zero, drain));
    if (e->nat_frames) {
        const size_t n_tab = devbuf_rule::nat_floats((size_t)n_nat, fdim);
        HIPCHK(r.nat.grow(n_tab, n_tab, e->bufs, zero, drain));
        HIPCHK(r.nat_row.grow(n_slots, n_slots, e->bufs, zero, drain));
    }
    *out = &r;
    return MLGGD_OK;
}

// the set just acquired and filled becomes the current indexed chunk: n samples over `rows` stream rows
static void raw_set_commit(mlggd_engine *e, int rows, int n, int ctx, int toff) {
    e->raw_cur ^= 1;
    e->nat = e->raw[e->raw_cur].nat.p;  // a decoding call then points it at its table of the whole batch
    e->chunk_frames = n;
    e->raw_frames = rows;
    e->indexed = true;
    e->fdim = stream_fdim(e, ctx);
    e->toff = toff;
}

// mlggd_load_frames and, on a NAT engine, mlggd_load_frames_nat (n_nat / nat / nat_row are read only there)
static int load_frames_impl(mlggd_engine *e, int n_frames, int fea_context, const float *feat, const float *targ,
                            int n_samples, const int32_t *first_frame, int targ_offset, int n_nat, const float *nat,
                            const int32_t *nat_row) {
    const bool natm = e->nat_frames > 0;
    const int fdim = stream_fdim(e, fea_context);
    if (fdim == 0 && natm)
        return fail(MLGGD_ERR_ARG, "(fea_context %d + 1) does not divide layersizes[0] = %d", fea_context, e->K0);
    if (fdim == 0) return fail(MLGGD_ERR_ARG, "fea_context %d does not divide layersizes[0] = %d", fea_context, e->K0);
    if (n_frames < 0 || n_samples < 0) return fail(MLGGD_ERR_ARG, "negative size");
    CHK(check_frames(e, n_samples));
    if (n_samples > 0 && (!feat || !first_frame)) return fail(MLGGD_ERR_ARG, "feat/first_frame is NULL");
    if (targ_offset < 0 || targ_offset >= fea_context)
        return fail(MLGGD_ERR_ARG, "targ_offset %d not in [0, fea_context)", targ_offset);
    for (int s = 0; s < n_samples; s++)
        if (first_frame[s] < 0 || first_frame[s] + fea_context > n_frames)
            return fail(MLGGD_ERR_ARG, "sample %d: window [%d,%d) outside the %d uploaded frames", s, first_frame[s],
                        first_frame[s] + fea_context, n_frames);
    if (natm) {
        if (n_nat < 0) return fail(MLGGD_ERR_ARG, "n_nat %d < 0", n_nat);
        if (n_samples > 0 && (!nat || !nat_row)) return fail(MLGGD_ERR_ARG, "nat/nat_row is NULL");
        for (int s = 0; s < n_samples; s++)
            if (nat_row[s] < 0 || nat_row[s] >= n_nat)
                return fail(MLGGD_ERR_ARG, "sample %d: nat_row %d outside the %d noise rows", s, nat_row[s], n_nat);
    }
    HIPCHK(hipSetDevice(e->device));
    // the set that is NOT current: copy beside whatever the main stream is still running
    mlggd_engine::RawSet *r;
    CHK(raw_set_acquire(e, n_frames, n_samples, fea_context, n_nat, true, &r));
    if (natm && n_samples > 0) {
        HIPCHK(hipMemcpyAsync(r->nat.p, nat, (size_t)n_nat * fdim * 4, hipMemcpyHostToDevice, e->copy_stream));
        HIPCHK(hipMemcpyAsync(r->nat_row.p, nat_row, (size_t)n_samples * sizeof(int), hipMemcpyHostToDevice, e->copy_stream));
    }
    if (n_frames > 0) {
        HIPCHK(hipMemcpyAsync(r->feat.p, feat, (size_t)n_frames * fdim * 4, hipMemcpyHostToDevice, e->copy_stream));
        if (targ) HIPCHK(hipMemcpyAsync(r->targ.p, targ, (size_t)n_frames * e->D * 4, hipMemcpyHostToDevice, e->copy_stream));
    }
    if (n_samples > 0)
        HIPCHK(hipMemcpyAsync(r->first.p, first_frame, (size_t)n_samples * sizeof(int), hipMemcpyHostToDevice, e->copy_stream));
    // the caller's buffers are free when this returns; kernels enqueued from now on see the data (the host has
    // observed the copies complete)
    HIPCHK(hipStreamSynchronize(e->copy_stream));
    raw_set_commit(e, n_frames, n_samples, fea_context, targ_offset);
    return MLGGD_OK;
}

// the _nat entries need a NAT engine, the plain frames entries one without
static int nat_entry_state(mlggd_engine *e, const char *who) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (e->nat_frames == 0) return fail(MLGGD_ERR_STATE, "%s needs an engine with nat_frames > 0", who);
    return MLGGD_OK;
}

extern "C" {

int mlggd_load_frames(mlggd_handle e, int n_frames, int fea_context, const float *feat, const float *targ,
                      int n_samples, const int32_t *first_frame, int targ_offset) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (e->nat_frames > 0)
        return fail(MLGGD_ERR_STATE, "the plain frames entries have no noise rows: an engine with nat_frames = %d takes "
                                     "mlggd_*_frames_nat", e->nat_frames);
    return load_frames_impl(e, n_frames, fea_context, feat, targ, n_samples, first_frame, targ_offset, 0, nullptr, nullptr);
}

int mlggd_load_frames_nat(mlggd_handle e, int n_frames, int fea_context, const float *feat, const float *targ,
                          int n_samples, const int32_t *first_frame, int targ_offset, int n_nat, const float *nat,
                          const int32_t *nat_row) {
    CHK(nat_entry_state(e, "mlggd_load_frames_nat"));
    return load_frames_impl(e, n_frames, fea_context, feat, targ, n_samples, first_frame, targ_offset, n_nat, nat, nat_row);
}

int mlggd_train_frames_nat(mlggd_handle e, int n_frames, int fea_context, const float *feat, const float *targ,
                           int n_samples, const int32_t *first_frame, int targ_offset, int n_nat, const float *nat,
                           const int32_t *nat_row, int *bunches_trained) {
    CHK(nat_entry_state(e, "mlggd_train_frames_nat"));
    if (n_samples > 0 && !targ) return fail(MLGGD_ERR_ARG, "targ is NULL");
    CHK(load_frames_impl(e, n_frames, fea_context, feat, targ, n_samples, first_frame, targ_offset, n_nat, nat, nat_row));
    CHK(mlggd_train_resident(e, 0, n_samples, bunches_trained));
    return mlggd_sync(e);
}

int mlggd_train_frames(mlggd_handle e, int n_frames, int fea_context, const float *feat, const float *targ,
                       int n_samples, const int32_t *first_frame, int targ_offset, int *bunches_trained) {
    if (n_samples > 0 && !targ) return fail(MLGGD_ERR_ARG, "targ is NULL");
    CHK(mlggd_load_frames(e, n_frames, fea_context, feat, targ, n_samples, first_frame, targ_offset));
    CHK(mlggd_train_resident(e, 0, n_samples, bunches_trained));
    return mlggd_sync(e);
}

// The same without the final wait: returns once the chunk is on the device (the caller's buffers are free) and
// its steps are enqueued.  The next call uploads the next chunk into the other device buffer set while these
// steps still run; mlggd_sync / mlggd_get_weights / any CV call waits for them.
int mlggd_train_frames_async(mlggd_handle e, int n_frames, int fea_context, const float *feat, const float *targ,
                             int n_samples, const int32_t *first_frame, int targ_offset, int *bunches_trained) {
    if (n_samples > 0 && !targ) return fail(MLGGD_ERR_ARG, "targ is NULL");
    CHK(mlggd_load_frames(e, n_frames, fea_context, feat, targ, n_samples, first_frame, targ_offset));
    return mlggd_train_resident(e, 0, n_samples, bunches_trained);
}

// Pinned host memory for the caller's chunk buffers (faster, truly asynchronous H2D).
int mlggd_alloc_pinned(size_t bytes, void **out) {
    if (!out) return fail(MLGGD_ERR_ARG, "out is NULL");
    HIPCHK(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return MLGGD_OK;
}
int mlggd_alloc_pinned_on(int device, size_t bytes, void **out) {
    if (!out) return fail(MLGGD_ERR_ARG, "out is NULL");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)  // the same message mlggd_create gives (BP_GPU.cu:17-21)
        return fail(MLGGD_ERR_ARG, "GPU Num %d Not In Range %d-%d", device, 0, ndev - 1);
    // the calling thread may have no current device yet (a host IO thread): pin through `device`'s context, then
    // put the thread's current device back so the call has no side effect on it
    int prev = -1;
    const bool had_prev = hipGetDevice(&prev) == hipSuccess;
    HIPCHK(hipSetDevice(device));
    const hipError_t err = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    if (had_prev && prev != device) hipSetDevice(prev);
    if (err != hipSuccess) return fail(MLGGD_ERR_DEVICE, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
    return MLGGD_OK;
}
int mlggd_free_pinned(void *p) {
    if (p) HIPCHK(hipHostFree(p));
    return MLGGD_OK;
}

int mlggd_train_resident(mlggd_handle e, int first_frame, int n_frames, int *bunches_trained) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (first_frame < 0 || n_frames < 0 || first_frame + n_frames > e->chunk_frames)
        return fail(MLGGD_ERR_ARG, "frames [%d,%d) outside the resident chunk of %d frames", first_frame,
                    first_frame + n_frames, e->chunk_frames);
    HIPCHK(hipSetDevice(e->device));
    int trained = 0;
    HIPCHK(hipEventRecord(e->ev_t0, e->stream));
    // bunch loop of BP_GPU::train, BP_GPU.cu:170-184: full bunches only
    bool prestaged = false;
    // an emulated world consumes one GLOBAL minibatch of world*B rows per step (and stages nothing ahead)
    const int per_step = e->fake_world ? e->B * e->world : e->B;
    for (int i = 0; i + per_step <= n_frames; i += per_step) {
        // (a NAT engine's frame stream is staged by k_transpose_in_nat in front of every step: the loss kernels'
        // ride-along staging gathers the plain window only)
        const bool has_next = e->stage_ahead && !e->fake_world && !(e->nat_frames && e->indexed) && i + 2 * e->B <= n_frames;
        Bunch next;
        if (has_next) next = bunch_at(e, first_frame + i + e->B);
        CHK(run_step(e, first_frame + i, prestaged, has_next ? &next : nullptr));
        prestaged = has_next;
        trained++;
    }
    HIPCHK(hipEventRecord(e->ev_t1, e->stream));
    if (e->indexed && e->copy_stream)  // the next-but-one upload reuses this buffer set: it waits for this point
        HIPCHK(hipEventRecord(e->raw[e->raw_cur].last_use, e->stream));
    e->last_steps = trained;
    e->timing_valid = true;
    if (bunches_trained) *bunches_trained = trained;
    return MLGGD_OK;
}

int mlggd_sync(mlggd_handle e) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->comm_stream) HIPCHK(hipStreamSynchronize(e->comm_stream));
    return MLGGD_OK;
}

int mlggd_train_chunk(mlggd_handle e, int n_frames, const float *in, const float *targ, int *bunches_trained) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (n_frames > 0 && (!in || !targ)) return fail(MLGGD_ERR_ARG, "in/targ is NULL");
    CHK(mlggd_load_chunk(e, n_frames, in, targ));
    CHK(mlggd_train_resident(e, 0, n_frames, bunches_trained));
    return mlggd_sync(e);  // BP_GPU.cu:439: train() returns after the last step completed
}

int mlggd_last_train_ms(mlggd_handle e, float *ms, int *steps) {
    if (!e || !ms) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (!e->timing_valid) return fail(MLGGD_ERR_STATE, "no mlggd_train_resident call to time");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipEventSynchronize(e->ev_t1));
    HIPCHK(hipEventElapsedTime(ms, e->ev_t0, e->ev_t1));
    if (steps) *steps = e->last_steps;
    return MLGGD_OK;
}

// Forward over a chunk whose inputs are resident: outputs into chunk_out[n][D].
static int forward_resident(mlggd_engine *e, int n_frames) {
    const size_t n_out = devbuf_rule::out_rows((size_t)n_frames) * e->D;
    HIPCHK(e->chunk_out.grow(n_out, n_out, e->bufs, nullptr, nullptr));
    const int b_tiles = e->Bp / 32;
    // bunch loop of CrossValid*, BP_GPU.cu:202-216: INCLUDES the trailing partial bunch
    for (int i = 0; i < n_frames; i += e->B) {
        const int fb = (e->B > n_frames - i) ? (n_frames - i) : e->B;
        CHK(run_forward(e, bunch_at(e, i), fb, false));
        hipLaunchKernelGGL(k_out_rowmajor, dim3((e->Dp / 32) * b_tiles), dim3(256), 0, e->stream, e->slab, e->S_out,
                           e->bias[e->L - 1], fb, e->D, e->Dp, e->Bp, e->chunk_out.p + (size_t)i * e->D, b_tiles);
        CHK(launch_check("k_out_rowmajor"));
    }
    return MLGGD_OK;
}

// ... and out [n][D] on the host when it returns (n = 0: nothing to do)
static int forward_to_host(mlggd_engine *e, int n, float *out) {
    if (n == 0) return MLGGD_OK;
    CHK(forward_resident(e, n));
    HIPCHK(hipMemcpyAsync(out, e->chunk_out.p, (size_t)n * e->D * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}

int mlggd_forward(mlggd_handle e, int n_frames, const float *in, float *out) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (n_frames > 0 && (!in || !out)) return fail(MLGGD_ERR_ARG, "in/out is NULL");
    CHK(mlggd_load_chunk(e, n_frames, in, nullptr));
    return forward_to_host(e, n_frames, out);
}

// BP_GPU::Gamma, BP_GPU.cu:593-640: 10th-order polynomial on (2,3] in double powers, each
// pair of terms rounded into a float accumulator; recurrences outside that interval.
float mlggd_gamma(float x) {
    static const float coef[11] = {0.0000677106, -0.0003442342, 0.0015397681, -0.0024467480, 0.0109736958,
                                   -0.0002109075, 0.0742379071, 0.0815782188,  0.4118402518,  0.4227843370,
                                   1.0000000000};
    if (x > 2 && x <= 3) {
        const double t = x - 2.0;
        float acc = 0;
        for (int i = 0; i < 8; i += 2) acc = acc + coef[i] * pow(t, 10.0 - i) + coef[i + 1] * pow(t, 9.0 - i);
        acc = acc + coef[8] * pow(t, 2.0) + coef[9] * t + coef[10];
        return acc;
    }
    if (x > 0 && x <= 1) return mlggd_gamma(x + 2) / (x * (x + 1));
    if (x > 1 && x <= 2) return mlggd_gamma(x + 1) / x;
    if (x > 3) {
        int i = 1;
        float prod = 1;
        while (!((x - i) > 2 && (x - i) <= 3)) {
            prod = (x - i) * prod;
            i++;
        }
        prod = prod * (x - i);
        return prod * mlggd_gamma(x - i);
    }
    return 0;
}

// Host accumulation exactly as CrossValid / CrossValiddB / CrossValid2 do it
// (BP_GPU.cu:207-213, 240-250, 271-301): fp32 scalars, frame-major order.  The chunk must be
// resident (expanded or indexed); target of sample i is trow(i).
static int cv_accumulate(mlggd_engine *e, int n_frames, const std::function<const float *(int)> &trow, float *sqerr,
                         float *abserr, float *loglik) {
    const int D = e->D;
    std::vector<float> out((size_t)n_frames * D);
    if (n_frames > 0) {
        CHK(forward_resident(e, n_frames));
        HIPCHK(hipMemcpyAsync(out.data(), e->chunk_out.p, (size_t)n_frames * D * 4, hipMemcpyDeviceToHost, e->stream));
    }
    std::vector<float> scalefac(D);
    if (loglik)
        HIPCHK(hipMemcpyAsync(scalefac.data(), e->scalefactor, (size_t)D * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (sqerr) {
        float s = 0.0f;
        for (int i = 0; i < n_frames; i++) {
            const float *t = trow(i), *o = &out[(size_t)i * D];
            for (int d = 0; d < D; d++) s = s + (o[d] - t[d]) * (o[d] - t[d]);
        }
        *sqerr = s;
    }
    if (abserr) {
        float s = 0.0f;
        for (int i = 0; i < n_frames; i++) {
            const float *t = trow(i), *o = &out[(size_t)i * D];
            for (int d = 0; d < D; d++) s = s + fabsf(o[d] - t[d]);
        }
        *abserr = s / D;
    }
    // the asymmetric model (asym_rule.h): s(o - t) in the place of |t - o| in density3, and density1 loses
    // n sum_d logf((kappa_d + 1/kappa_d) / 2), the D fp32 logarithms added in double; exactly 0 at kappa = 1
    const float *kap = e->asym ? e->kappas_host.data() : nullptr;
    double kterm = 0;
    if (loglik && kap) {
        for (int d = 0; d < D; d++) kterm += (double)asym_rule::log_norm(kap[d]);
        kterm = kterm * n_frames;
    }
    if (loglik && e->per_bin) {  // the same three terms with beta_d; density1 is a sum over the bins, kept in double
        const float *betas = e->betas_host.data();
        double d1 = 0;
        for (int d = 0; d < D; d++) d1 += (double)n_frames * logf(betas[d] / (2 * mlggd_gamma((float)(1.0 / betas[d]))));
        if (kap) d1 = d1 - kterm;
        float density2 = 0, density3 = 0;
        for (int u = 0; u < D; u++) density2 += logf(scalefac[u]);
        density2 = density2 * n_frames;
        for (int i = 0; i < n_frames; i++) {
            const float *t = trow(i), *o = &out[(size_t)i * D];
            for (int d = 0; d < D; d++) {
                const float err = t[d] - o[d];
                density3 += powf((kap ? asym_rule::skewed(o[d] - t[d], kap[d]) : fabsf(err)) / scalefac[d], betas[d]);
            }
        }
        *loglik = (float)d1 - density2 - density3;
    } else if (loglik) {
        const float beta = e->cfg.shapefactor;
        float density1, density2 = 0, density3 = 0;
        density1 = n_frames * D * logf(beta / (2 * mlggd_gamma((float)(1.0 / beta))));
        if (kap) density1 = density1 - (float)kterm;
        for (int u = 0; u < D; u++) density2 += logf(scalefac[u]);
        density2 = density2 * n_frames;
        for (int i = 0; i < n_frames; i++) {
            const float *t = trow(i), *o = &out[(size_t)i * D];
            for (int d = 0; d < D; d++) {
                const float err = t[d] - o[d];
                density3 += powf((kap ? asym_rule::skewed(o[d] - t[d], kap[d]) : fabsf(err)) / scalefac[d], beta);
            }
        }
        *loglik = density1 - density2 - density3;
    }
    return MLGGD_OK;
}

// The same three numbers with the sums formed on the device (mlggd_set_cv_device_reduce): one
// forward pass, k_cv_reduce per bunch, 3 doubles per 32x32 tile copied back -- no n x D transfer and no host
// loop.  The chunk (inputs AND targets) must be resident.
static int cv_device_reduce(mlggd_engine *e, int n_frames, float *sqerr, float *abserr, float *loglik) {
    const int D = e->D, b_tiles = e->Bp / 32, tiles = (e->Dp / 32) * b_tiles;
    const int nb = (n_frames + e->B - 1) / e->B;
    const size_t need = (size_t)(nb > 0 ? nb : 1) * tiles * 3;
    HIPCHK(e->cv_partial.grow(need, need, e->bufs, nullptr, nullptr));
    const ErrModelInUse em = err_model(e);
    CvArgs a;
    a.slab = e->slab; a.S = e->S_out; a.bias = e->bias[e->L - 1];
    a.D = D; a.Dp = e->Dp; a.Bp = e->Bp; a.beta = e->cfg.shapefactor;
    a.alpha = loglik ? e->scalefactor : nullptr;
    a.toff = e->toff; a.b_tiles = b_tiles;
    CHK(walk_bunches(e, n_frames, [&](const Bunch &bn, int fb, int k) {
        a.targ = bn.targ; a.first = bn.first; a.B = fb;
        a.partial = e->cv_partial.p + (size_t)k * tiles * 3;
        switch (loglik ? em.model : EM_SHARED) {  // the models differ in the likelihood term only
        case EM_ASYM: return launch_loss(e, "k_cv_reduce_asym", k_cv_reduce_asym, dim3(tiles), dim3(256), 0, 0, a, em.betas, em.kappas);
        case EM_BINS: return launch_loss(e, "k_cv_reduce_bins", k_cv_reduce_bins, dim3(tiles), dim3(256), 0, 0, a, em.betas);
        default: return launch_loss(e, "k_cv_reduce", k_cv_reduce, dim3(tiles), dim3(256), 0, 0, a);
        }
    }));
    std::vector<double> part((size_t)nb * tiles * 3);
    std::vector<float> scalefac(D);
    if (nb > 0)
        HIPCHK(hipMemcpyAsync(part.data(), e->cv_partial.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (loglik) HIPCHK(hipMemcpyAsync(scalefac.data(), e->scalefactor, (size_t)D * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    double s[3] = {0, 0, 0};
    for (size_t i = 0; i < part.size(); i += 3)
        for (int j = 0; j < 3; j++) s[j] += part[i + j];
    if (sqerr) *sqerr = (float)s[0];
    if (abserr) *abserr = (float)(s[1] / D);
    if (loglik) {  // density1 - density2 - density3, BP_GPU.cu:271-301
        const float beta = e->cfg.shapefactor;
        double density1 = (double)n_frames * D * logf(beta / (2 * mlggd_gamma((float)(1.0 / beta))));
        if (e->per_bin) {
            density1 = 0;
            for (int d = 0; d < D; d++) {
                const float bd = e->betas_host[d];
                density1 += (double)n_frames * logf(bd / (2 * mlggd_gamma((float)(1.0 / bd))));
            }
        }
        if (e->asym) {  // minus n sum_d logf((kappa_d + 1/kappa_d) / 2), exactly 0 at kappa = 1 (asym_rule.h)
            double kterm = 0;
            for (int d = 0; d < D; d++) kterm += (double)asym_rule::log_norm(e->kappas_host[d]);
            density1 = density1 - kterm * n_frames;
        }
        double density2 = 0;
        for (int u = 0; u < D; u++) density2 += logf(scalefac[u]);
        *loglik = (float)(density1 - density2 * n_frames - s[2]);
    }
    return MLGGD_OK;
}

static int cv_metrics(mlggd_engine *e, int n_frames, const float *in, const float *targ, float *sqerr, float *abserr,
                      float *loglik) {
    if (n_frames > 0 && (!in || !targ)) return fail(MLGGD_ERR_ARG, "in/targ is NULL");
    if (e->cv_device) {
        CHK(mlggd_load_chunk(e, n_frames, in, targ));
        return cv_device_reduce(e, n_frames, sqerr, abserr, loglik);
    }
    CHK(mlggd_load_chunk(e, n_frames, in, nullptr));
    const int D = e->D;
    return cv_accumulate(e, n_frames, [&](int i) { return targ + (size_t)i * D; }, sqerr, abserr, loglik);
}

int mlggd_cv_sqerr(mlggd_handle e, int n, const float *in, const float *targ, float *out) {
    if (!e || !out) return fail(MLGGD_ERR_ARG, "NULL argument");
    return cv_metrics(e, n, in, targ, out, nullptr, nullptr);
}
int mlggd_cv_abserr(mlggd_handle e, int n, const float *in, const float *targ, float *out) {
    if (!e || !out) return fail(MLGGD_ERR_ARG, "NULL argument");
    return cv_metrics(e, n, in, targ, nullptr, out, nullptr);
}
int mlggd_cv_loglik(mlggd_handle e, int n, const float *in, const float *targ, float *out) {
    if (!e || !out) return fail(MLGGD_ERR_ARG, "NULL argument");
    return cv_metrics(e, n, in, targ, nullptr, nullptr, out);
}
int mlggd_cv_all(mlggd_handle e, int n, const float *in, const float *targ, float *sqerr, float *abserr,
                 float *loglik) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    return cv_metrics(e, n, in, targ, sqerr, abserr, (e->cfg.MLflag == 1) ? loglik : nullptr);
}

// the three numbers of the indexed chunk that is current: the sums formed on the device read the set's own targets,
// the host-order sums read host_targ [.][D], in both cases row first_frame[i] + targ_offset for sample i
static int cv_indexed(mlggd_engine *e, int n_samples, const int32_t *first_frame, int targ_offset, const float *host_targ,
                      float *sqerr, float *abserr, float *loglik) {
    float *ll = (e->cfg.MLflag == 1) ? loglik : nullptr;
    if (e->cv_device) return cv_device_reduce(e, n_samples, sqerr, abserr, ll);
    const int D = e->D;
    return cv_accumulate(
        e, n_samples, [&](int i) { return host_targ + (size_t)(first_frame[i] + targ_offset) * D; }, sqerr, abserr, ll);
}

int mlggd_cv_all_frames_nat(mlggd_handle e, int n_frames, int fea_context, const float *feat, const float *targ,
                            int n_samples, const int32_t *first_frame, int targ_offset, int n_nat, const float *nat,
                            const int32_t *nat_row, float *sqerr, float *abserr, float *loglik) {
    CHK(nat_entry_state(e, "mlggd_cv_all_frames_nat"));
    if (n_samples > 0 && !targ) return fail(MLGGD_ERR_ARG, "targ is NULL");
    CHK(load_frames_impl(e, n_frames, fea_context, feat, e->cv_device ? targ : nullptr, n_samples, first_frame,
                         targ_offset, n_nat, nat, nat_row));
    return cv_indexed(e, n_samples, first_frame, targ_offset, targ, sqerr, abserr, loglik);
}

int mlggd_forward_frames_nat(mlggd_handle e, int n_frames, int fea_context, const float *feat, int n_samples,
                             const int32_t *first_frame, int n_nat, const float *nat, const int32_t *nat_row,
                             float *out) {
    CHK(nat_entry_state(e, "mlggd_forward_frames_nat"));
    if (n_samples > 0 && !out) return fail(MLGGD_ERR_ARG, "out is NULL");
    CHK(load_frames_impl(e, n_frames, fea_context, feat, nullptr, n_samples, first_frame, 0, n_nat, nat, nat_row));
    return forward_to_host(e, n_samples, out);
}

// Host only, no device (nat_rule.h): the noise rows of n_utts utterances from their normalised rows, and the utterance
// of every sample.
int mlggd_nat_estimate(int D, int n_utts, const int32_t *frame_off, const float *rows, int nat_frames, float *out) {
    if (D < 1) return fail(MLGGD_ERR_ARG, "D %d < 1", D);
    if (n_utts < 0) return fail(MLGGD_ERR_ARG, "n_utts %d < 0", n_utts);
    if (nat_frames < 1) return fail(MLGGD_ERR_ARG, "nat_frames %d < 1", nat_frames);
    if (n_utts == 0) return MLGGD_OK;
    if (!frame_off || !out) return fail(MLGGD_ERR_ARG, "frame_off/out is NULL");
    for (int u = 0; u < n_utts; u++)
        if (frame_off[u] < 0 || frame_off[u + 1] < frame_off[u])
            return fail(MLGGD_ERR_ARG, "frame_off decreases at utterance %d (%d after %d)", u, frame_off[u + 1], frame_off[u]);
    if (frame_off[n_utts] > frame_off[0] && !rows) return fail(MLGGD_ERR_ARG, "rows is NULL");
    for (int u = 0; u < n_utts; u++) {
        const int Tu = nat_rule::frames_used(nat_frames, frame_off[u + 1] - frame_off[u]);
        for (int k = 0; k < D; k++)
            out[(size_t)u * D + k] = Tu ? nat_rule::chain(rows + (size_t)frame_off[u] * D + k, (size_t)D, Tu) : 0.0f;
    }
    return MLGGD_OK;
}

int mlggd_nat_rows(int n_utts, const int32_t *frame_off, int n_samples, const int32_t *first_frame, int32_t *nat_row) {
    if (n_utts < 0 || n_samples < 0) return fail(MLGGD_ERR_ARG, "negative size");
    if (n_samples == 0) return MLGGD_OK;
    if (!frame_off || !first_frame || !nat_row) return fail(MLGGD_ERR_ARG, "frame_off/first_frame/nat_row is NULL");
    for (int u = 0; u < n_utts; u++)
        if (frame_off[u] < 0 || frame_off[u + 1] < frame_off[u])
            return fail(MLGGD_ERR_ARG, "frame_off decreases at utterance %d (%d after %d)", u, frame_off[u + 1], frame_off[u]);
    const int FT = n_utts ? frame_off[n_utts] : 0, F0 = n_utts ? frame_off[0] : 0;
    for (int s = 0; s < n_samples; s++) {
        if (first_frame[s] < F0 || first_frame[s] >= FT)
            return fail(MLGGD_ERR_ARG, "sample %d: frame %d outside the %d packed frames", s, first_frame[s], FT);
        nat_row[s] = nat_rule::utt_of_frame(n_utts, frame_off, first_frame[s]);
    }
    return MLGGD_OK;
}

int mlggd_get_nat_frames(mlggd_handle e, int *nat_frames) {
    if (!e || !nat_frames) return fail(MLGGD_ERR_ARG, "NULL argument");
    *nat_frames = e->nat_frames;
    return MLGGD_OK;
}

int mlggd_cv_all_frames(mlggd_handle e, int n_frames, int fea_context, const float *feat, const float *targ,
                        int n_samples, const int32_t *first_frame, int targ_offset, float *sqerr, float *abserr,
                        float *loglik) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (n_samples > 0 && !targ) return fail(MLGGD_ERR_ARG, "targ is NULL");
    CHK(mlggd_load_frames(e, n_frames, fea_context, feat, e->cv_device ? targ : nullptr, n_samples, first_frame,
                          targ_offset));
    return cv_indexed(e, n_samples, first_frame, targ_offset, targ, sqerr, abserr, loglik);
}

int mlggd_forward_frames(mlggd_handle e, int n_frames, int fea_context, const float *feat, int n_samples,
                         const int32_t *first_frame, float *out) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (n_samples > 0 && !out) return fail(MLGGD_ERR_ARG, "out is NULL");
    CHK(mlggd_load_frames(e, n_frames, fea_context, feat, nullptr, n_samples, first_frame, 0));
    return forward_to_host(e, n_samples, out);
}

// ------------------------------------------------------------------ column statistics (colstats.hip.h)
static int check_betas(int n_betas, const float *betas) {
    if (n_betas < 1 || n_betas > MLGGD_MAX_BETAS)
        return fail(MLGGD_ERR_ARG, "n_betas %d not in 1..%d", n_betas, MLGGD_MAX_BETAS);
    if (!betas) return fail(MLGGD_ERR_ARG, "betas is NULL");
    for (int k = 0; k < n_betas; k++)
        if (!(betas[k] > 0.0f) || !std::isfinite(betas[k]))
            return fail(MLGGD_ERR_ARG, "betas[%d] = %g: a shape must be positive and finite", k, (double)betas[k]);
    return MLGGD_OK;
}
static int error_stats_state(mlggd_engine *e, const char *who, const char *what) {
    if (e->comm || e->fake_world) return fail(MLGGD_ERR_STATE, "%s runs on a single-device engine", who);
    if (e->cfg.dropoutflag != 0)
        return fail(MLGGD_ERR_STATE, "%s: %s not available with dropoutflag = %d", who, what, e->cfg.dropoutflag);
    return MLGGD_OK;
}
// One call of the three statistics: which terms, the call's grid (none for the output statistics) and where the sums
// go.  None of them looks at the skew or shape vector in effect: the statistics are of the errors, the grid is the call's.
enum ColStatsKind { COLSTATS_ERR, COLSTATS_ERR_SIGNED, COLSTATS_OUT };
struct ColStatsCall {
    ColStatsKind kind;
    int n_betas;
    const float *betas;
    double *sums;  // [rows()][D]
    bool grid() const { return kind != COLSTATS_OUT; }
    int rows(int K) const { return kind == COLSTATS_ERR ? 4 + K : kind == COLSTATS_ERR_SIGNED ? 2 * K : gv_rule::kRows; }
    int rows() const { return rows(n_betas); }
    const char *what() const { return grid() ? "the error model is" : "the output statistics are"; }
};
// k_err_stats into es_acc, [4 + n_betas][D]; k_err_stats_signed into ess_acc, [2 n_betas][D], the rows of P+ then of
// P-; k_out_stats into os_acc, [4][D].  The error accumulators are sized for the largest grid.
static int col_stats_run(mlggd_engine *e, int n, const ColStatsCall &c) {
    const size_t n_acc = (size_t)c.rows(MLGGD_MAX_BETAS) * e->D;
    if (c.kind == COLSTATS_OUT)
        return col_stats_resident(e, n, e->os_acc, n_acc, c.rows(), k_out_stats, "k_out_stats", OutStatsArgs(), c.sums);
    ErrStatsArgs a;
    a.K = c.n_betas;
    for (int k = 0; k < MLGGD_MAX_BETAS; k++) a.betas[k] = k < c.n_betas ? c.betas[k] : 1.0f;
    return c.kind == COLSTATS_ERR_SIGNED
               ? col_stats_resident(e, n, e->ess_acc, n_acc, c.rows(), k_err_stats_signed, "k_err_stats_signed", a, c.sums)
               : col_stats_resident(e, n, e->es_acc, n_acc, c.rows(), k_err_stats, "k_err_stats", a, c.sums);
}
static int col_stats_zero(mlggd_engine *e, const ColStatsCall &c) {
    std::fill(c.sums, c.sums + (size_t)c.rows() * e->D, 0.0);
    return MLGGD_OK;
}
// The two forms of the six entries.  The order of the checks decides which error wins and is the entries' contract.
static int col_stats_chunk(mlggd_engine *e, const char *who, const ColStatsCall &c, int n_frames, const float *in,
                           const float *targ) {
    if (!e || !c.sums) return fail(MLGGD_ERR_ARG, "NULL handle / sums");
    if (c.grid()) CHK(check_betas(c.n_betas, c.betas));
    CHK(check_frames(e, n_frames));
    if (n_frames > 0 && (!in || !targ)) return fail(MLGGD_ERR_ARG, "in/targ is NULL");
    CHK(error_stats_state(e, who, c.what()));
    if (n_frames == 0) return col_stats_zero(e, c);
    CHK(mlggd_load_chunk(e, n_frames, in, targ));
    return col_stats_run(e, n_frames, c);
}
static int col_stats_frames(mlggd_engine *e, const char *who, const ColStatsCall &c, int n_frames, int fea_context,
                            const float *feat, const float *targ, int n_samples, const int32_t *first_frame,
                            int targ_offset) {
    if (!e || !c.sums) return fail(MLGGD_ERR_ARG, "NULL handle / sums");
    if (c.grid()) CHK(check_betas(c.n_betas, c.betas));
    if (n_samples > 0 && !targ) return fail(MLGGD_ERR_ARG, "targ is NULL");
    CHK(error_stats_state(e, who, c.what()));
    // the remaining shape checks are mlggd_load_frames' own, all made before its first device call
    CHK(mlggd_load_frames(e, n_frames, fea_context, feat, targ, n_samples, first_frame, targ_offset));
    if (n_samples == 0) return col_stats_zero(e, c);
    return col_stats_run(e, n_samples, c);
}

int mlggd_error_stats(mlggd_handle e, int n_frames, const float *in, const float *targ, int n_betas,
                      const float *betas, double *sums) {
    return col_stats_chunk(e, "mlggd_error_stats", {COLSTATS_ERR, n_betas, betas, sums}, n_frames, in, targ);
}
int mlggd_error_stats_frames(mlggd_handle e, int n_frames, int fea_context, const float *feat, const float *targ,
                             int n_samples, const int32_t *first_frame, int targ_offset, int n_betas,
                             const float *betas, double *sums) {
    return col_stats_frames(e, "mlggd_error_stats_frames", {COLSTATS_ERR, n_betas, betas, sums}, n_frames, fea_context, feat,
                            targ, n_samples, first_frame, targ_offset);
}
int mlggd_error_stats_signed(mlggd_handle e, int n_frames, const float *in, const float *targ, int n_betas,
                             const float *betas, double *sums) {
    return col_stats_chunk(e, "mlggd_error_stats_signed", {COLSTATS_ERR_SIGNED, n_betas, betas, sums}, n_frames, in, targ);
}
int mlggd_error_stats_signed_frames(mlggd_handle e, int n_frames, int fea_context, const float *feat, const float *targ,
                                    int n_samples, const int32_t *first_frame, int targ_offset, int n_betas,
                                    const float *betas, double *sums) {
    return col_stats_frames(e, "mlggd_error_stats_signed_frames", {COLSTATS_ERR_SIGNED, n_betas, betas, sums}, n_frames,
                            fea_context, feat, targ, n_samples, first_frame, targ_offset);
}
int mlggd_output_stats(mlggd_handle e, int n_frames, const float *in, const float *targ, double *sums) {
    return col_stats_chunk(e, "mlggd_output_stats", {COLSTATS_OUT, 0, nullptr, sums}, n_frames, in, targ);
}
int mlggd_output_stats_frames(mlggd_handle e, int n_frames, int fea_context, const float *feat, const float *targ,
                              int n_samples, const int32_t *first_frame, int targ_offset, double *sums) {
    return col_stats_frames(e, "mlggd_output_stats_frames", {COLSTATS_OUT, 0, nullptr, sums}, n_frames, fea_context, feat,
                            targ, n_samples, first_frame, targ_offset);
}

// Host only, no device: the closed-form fit of the asymmetric model (asym_rule::fit) for every bin and grid shape from
// the sums of mlggd_error_stats_signed.  Everything in double; ties go to the lower index; a bin with P+ == 0 or
// P- == 0 at a shape has no fit there and stays out of that shape's shared total.
int mlggd_asym_fit(int D, int64_t n, int n_betas, const float *betas, const double *signed_sums, double *kappa,
                   double *alpha, double *loglik, int32_t *best, double *loglik_shared, int32_t *best_shared) {
    if (D < 1) return fail(MLGGD_ERR_ARG, "D %d < 1", D);
    if (n <= 0) return fail(MLGGD_ERR_ARG, "n %lld: the fit needs at least one sample", (long long)n);
    CHK(check_betas(n_betas, betas));
    if (!signed_sums) return fail(MLGGD_ERR_ARG, "signed_sums is NULL");
    std::vector<double> shared(n_betas, 0.0);
    bool any = false;
    for (int d = 0; d < D; d++) {
        int arg = -1;
        double top = 0.0;
        for (int k = 0; k < n_betas; k++) {
            const asym_rule::Fit f = asym_rule::fit(signed_sums[(size_t)k * D + d], signed_sums[(size_t)(n_betas + k) * D + d],
                                                    (double)betas[k], (double)n);
            if (f.fitted) {
                shared[k] += f.loglik;
                any = true;
                if (arg < 0 || f.loglik > top) {
                    arg = k;
                    top = f.loglik;
                }
            }
            if (kappa) kappa[(size_t)k * D + d] = f.kappa;
            if (alpha) alpha[(size_t)k * D + d] = f.alpha;
            if (loglik) loglik[(size_t)k * D + d] = f.loglik;
        }
        if (best) best[d] = arg;
    }
    int arg = -1;
    if (any)
        for (int k = 0; k < n_betas; k++)
            if (arg < 0 || shared[k] > shared[arg]) arg = k;
    if (loglik_shared) std::copy(shared.begin(), shared.end(), loglik_shared);
    if (best_shared) *best_shared = arg;
    return MLGGD_OK;
}

// Host only, no device: moments, ML scale and profile log-likelihood of the GGD error model from the sums of
// mlggd_error_stats.  Everything in double; lgamma is libm's (the reference's polynomial Gamma, mlggd_gamma, stays
// with the log lines it belongs to).
int mlggd_ggd_fit(int D, int64_t n, int n_betas, const float *betas, const double *sums, double *mean, double *var,
                  double *kurt, double *alpha, double *loglik, int32_t *best, double *loglik_shared,
                  int32_t *best_shared) {
    if (D < 1) return fail(MLGGD_ERR_ARG, "D %d < 1", D);
    if (n <= 0) return fail(MLGGD_ERR_ARG, "n %lld: the fit needs at least one sample", (long long)n);
    CHK(check_betas(n_betas, betas));
    if (!sums) return fail(MLGGD_ERR_ARG, "sums is NULL");
    const double nn = (double)n, nan = std::nan("");
    std::vector<double> shared(n_betas, 0.0);
    for (int d = 0; d < D; d++) {
        const double s1 = sums[d], s2 = sums[(size_t)D + d], s3 = sums[(size_t)2 * D + d], s4 = sums[(size_t)3 * D + d];
        const bool fit = s2 != 0.0;  // every error of the bin is zero: no scale, no likelihood
        const double mu = s1 / nn, r2 = s2 / nn, r3 = s3 / nn, r4 = s4 / nn;
        const double m2 = r2 - mu * mu;
        const double m4 = ((r4 - 4.0 * mu * r3) + 6.0 * (mu * mu) * r2) - 3.0 * ((mu * mu) * (mu * mu));
        if (mean) mean[d] = mu;
        if (var) var[d] = m2;
        if (kurt) kurt[d] = fit ? m4 / (m2 * m2) - 3.0 : nan;
        int arg = -1;
        double top = 0.0;
        for (int k = 0; k < n_betas; k++) {
            const double b = (double)betas[k];
            double a = 0.0, l = nan;
            if (fit) {
                const double lna = log(b * sums[(size_t)(4 + k) * D + d] / nn) / b;  // alpha^beta = beta P / n
                a = exp(lna);
                l = nn * ((((log(b) - log(2.0)) - lgamma(1.0 / b)) - lna) - 1.0 / b);
                shared[k] += l;
                if (arg < 0 || l > top) {
                    arg = k;
                    top = l;
                }
            }
            if (alpha) alpha[(size_t)k * D + d] = a;
            if (loglik) loglik[(size_t)k * D + d] = l;
        }
        if (best) best[d] = arg;
    }
    int arg = -1;
    bool any = false;
    for (int d = 0; d < D; d++) any = any || sums[(size_t)D + d] != 0.0;
    if (any)
        for (int k = 0; k < n_betas; k++)
            if (arg < 0 || shared[k] > shared[arg]) arg = k;
    if (loglik_shared) std::copy(shared.begin(), shared.end(), loglik_shared);
    if (best_shared) *best_shared = arg;
    return MLGGD_OK;
}

// row-major [B][N] on the host from a device activation buffer: [Bp][Np], or owner-blocked [world][Bp][yb] (yb > 0:
// the all-to-all form's Y_l and staged rows)
static int rows_to_host(mlggd_engine *e, const float *src, int N, int Np, int yb, float *dst) {
    const int B = e->B, Bp = e->Bp;
    std::vector<float> t(yb ? (size_t)e->world * Bp * yb : (size_t)Bp * Np);
    HIPCHK(hipMemcpyAsync(t.data(), src, t.size() * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int b = 0; b < B; b++)
        for (int n = 0; n < N; n++)
            dst[(size_t)b * N + n] = yb ? t[(size_t)(n / yb) * Bp * yb + (size_t)b * yb + n % yb] : t[(size_t)b * Np + n];
    return MLGGD_OK;
}
// [B][D] on the host from outT [Dp][Bp]
static int out_to_host(mlggd_engine *e, const float *outT, float *dst) {
    std::vector<float> t((size_t)e->Dp * e->Bp);
    HIPCHK(hipMemcpyAsync(t.data(), outT, t.size() * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int b = 0; b < e->B; b++)
        for (int d = 0; d < e->D; d++) dst[(size_t)b * e->D + d] = t[(size_t)d * e->Bp + b];
    return MLGGD_OK;
}

int mlggd_debug_tensor(mlggd_handle e, const char *name, int layer, float *dst, size_t count) {
    if (!e || !name || !dst) return fail(MLGGD_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(e->device));
    const int L = e->L, B = e->B, Bp = e->Bp;
    const std::string nm(name);
    auto need = [&](size_t n) -> int {
        return count < n ? fail(MLGGD_ERR_ARG, "dst holds %zu floats, %s needs %zu", count, name, n) : MLGGD_OK;
    };
    if (nm == "scalefactor") {
        CHK(need(e->D));
        return mlggd_get_scalefactor(e, dst);
    }
    if (nm == "out") {  // outT [Dp][Bp] -> [B][D]
        CHK(need((size_t)B * e->D));
        return out_to_host(e, e->outT, dst);
    }
    if (layer < 1 || layer >= L) return fail(MLGGD_ERR_ARG, "layer %d not in 1..%d", layer, L - 1);
    const int N = e->ls[layer], Np = e->lsp[layer], K = e->ls[layer - 1];
    if (nm == "y" || nm == "dedx" || nm == "yt" || nm == "dedxt") {
        const bool tr = (nm == "yt" || nm == "dedxt");
        const float *src = (nm == "y") ? e->Y[layer] : (nm == "dedx") ? e->dEdX[layer]
                           : (nm == "yt") ? e->Yt[layer] : e->dEdXt[layer];
        if (!src) return fail(MLGGD_ERR_ARG, "%s not kept for layer %d", name, layer);
        CHK(need((size_t)B * N));
        if (!tr) return rows_to_host(e, src, N, Np, (nm == "y" && e->dp_a2a && layer < L - 1) ? e->shard_rows[layer + 1] * 64 : 0, dst);
        std::vector<float> t((size_t)Np * Bp);
        HIPCHK(hipMemcpyAsync(t.data(), src, t.size() * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (int b = 0; b < B; b++)
            for (int n = 0; n < N; n++) dst[(size_t)b * N + n] = t[(size_t)n * Bp + b];
        return MLGGD_OK;
    }
    if (nm == "weights" || nm == "delta_w" || nm == "grad_w") {
        CHK(wait_weight_gathers(e, 1, L - 1));
        const float *src = (nm == "weights") ? e->W[layer] : (nm == "delta_w") ? e->dW[layer] : e->G[layer];
        if (!src) return fail(MLGGD_ERR_STATE, "tensor %s does not exist on this path", name);
        if (!src) return fail(MLGGD_ERR_ARG, "%s not kept for layer %d", name, layer);
        CHK(need((size_t)K * N));
        CHK(download_padded(dst, src, Np, K, N, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return MLGGD_OK;
    }
    if (nm == "grad_b") {
        if (!e->gb[layer]) return fail(MLGGD_ERR_STATE, "tensor %s does not exist on this path", name);
        CHK(need(N));
        HIPCHK(hipMemcpyAsync(dst, e->gb[layer], (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return MLGGD_OK;
    }
    if (nm == "adam_pads") {  // how many pad entries of W, m_w, v_w, bias, m_b, v_b of the layer are not (+-)0: [6]
        if (e->opt_kind != MLGGD_OPT_ADAM) return fail(MLGGD_ERR_STATE, "tensor %s does not exist on this path", name);
        CHK(need(6));
        const int Kp = e->lsp[layer - 1];
        const float *mats[3] = {e->W[layer], e->adam_mw[layer].p, e->adam_vw[layer].p};
        const float *vecs[3] = {e->bias[layer], e->adam_mb[layer].p, e->adam_vb[layer].p};
        std::vector<float> t((size_t)Kp * Np);
        for (int a = 0; a < 3; a++) {
            HIPCHK(hipMemcpyAsync(t.data(), mats[a], t.size() * 4, hipMemcpyDeviceToHost, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
            size_t bad = 0;
            for (int k = 0; k < Kp; k++)
                for (int n = 0; n < Np; n++) bad += (k >= K || n >= N) && t[(size_t)k * Np + n] != 0.0f;
            dst[a] = (float)bad;
            HIPCHK(hipMemcpyAsync(t.data(), vecs[a], (size_t)Np * 4, hipMemcpyDeviceToHost, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
            bad = 0;
            for (int n = N; n < Np; n++) bad += t[n] != 0.0f;
            dst[3 + a] = (float)bad;
        }
        return MLGGD_OK;
    }
    if (nm == "bias" || nm == "delta_b") {
        CHK(need(N));
        HIPCHK(hipMemcpyAsync(dst, nm == "bias" ? e->bias[layer] : e->dbias[layer], (size_t)N * 4,
                              hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return MLGGD_OK;
    }
    return fail(MLGGD_ERR_ARG, "unknown tensor name '%s'", name);
}

int mlggd_debug_keep_ranks(mlggd_handle e, int on) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    HIPCHK(hipSetDevice(e->device));
    e->keep_ranks = on != 0;
    return keep_alloc(e);
}

int mlggd_debug_rank_tensor(mlggd_handle e, const char *name, int layer, int rank, float *dst, size_t count) {
    if (!e || !name || !dst) return fail(MLGGD_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(e->device));
    const int L = e->L, B = e->B;
    const std::string nm(name);
    if (rank < 0 || rank >= e->world) return fail(MLGGD_ERR_ARG, "rank %d not in 0..%d", rank, e->world - 1);
    // the rank whose step ran last in this process reads the live buffers; an emulated earlier rank its snapshot
    const bool live = rank == (e->fake_world ? e->world - 1 : e->rank);
    if (!live && (!e->fake_world || (size_t)rank >= e->snap_x.size()))
        return fail(MLGGD_ERR_STATE, "rank %d: only emulated ranks are kept (mlggd_debug_keep_ranks before training)", rank);
    auto need = [&](size_t n) -> int {
        return count < n ? fail(MLGGD_ERR_ARG, "dst holds %zu floats, %s needs %zu", count, name, n) : MLGGD_OK;
    };
    if (nm == "out") {
        CHK(need((size_t)B * e->D));
        return out_to_host(e, live ? e->outT : e->snap_out[rank], dst);
    }
    if (nm == "x") {
        CHK(need((size_t)B * e->ls[0]));
        return rows_to_host(e, live ? e->in_bunch : e->snap_x[rank], e->ls[0], e->lsp[0], e->dp_a2a ? e->shard_rows[1] * 64 : 0, dst);
    }
    if (nm == "y" || nm == "dedx") {
        const bool y = nm == "y";
        if (layer < 1 || layer >= (y ? L - 1 : L)) return fail(MLGGD_ERR_ARG, "%s: layer %d not in 1..%d", name, layer, y ? L - 2 : L - 1);
        CHK(need((size_t)B * e->ls[layer]));
        const float *src = y ? (live ? e->Y[layer] : e->snap_y[layer][rank]) : (live ? e->dEdX[layer] : e->snap_dedx[layer][rank]);
        return rows_to_host(e, src, e->ls[layer], e->lsp[layer], (y && e->dp_a2a) ? e->shard_rows[layer + 1] * 64 : 0, dst);
    }
    return fail(MLGGD_ERR_ARG, "unknown tensor name '%s'", name);
}

// ---- data parallel
// gradient buffers (layer_ydedx / layer_sumdedx of BP_WorkSpace) only exist on the all-reduce path
static int shard_alloc(mlggd_engine *e);
static int allreduce_alloc(mlggd_engine *e) {
    // reduce-scatter form: the block table of the sharded factor mode (shard_rows[l] tile rows per rank, W_l grown
    // to world x block rows, one event per layer for the W all-gathers); G_l gets the same rows so that every rank's
    // block of the reduce-scatter has the same size (rows past Kp are never written: they stay zero)
    if (e->ar_shard) CHK(shard_alloc(e));
    size_t gbn = 0;
    for (int l = 1; l < e->L; l++) gbn += e->lsp[l];
    CHK(dev_alloc(e, &e->gb_all, gbn));
    e->gb_all_count = gbn;
    size_t off = 0;
    for (int l = e->L - 1; l >= 1; l--) {
        const size_t rows = e->ar_shard ? (size_t)e->shard_rows[l] * 64 * e->world : (size_t)e->lsp[l - 1];
        CHK(dev_alloc(e, &e->G[l], (rows > (size_t)e->lsp[l - 1] ? rows : (size_t)e->lsp[l - 1]) * e->lsp[l]));
        e->gb[l] = e->gb_all + off;
        off += e->lsp[l];
        HIPCHK(hipEventCreateWithFlags(&e->ev_grad[l], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&e->ev_red[l], hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&e->ev_bias, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&e->ev_bias_red, hipEventDisableTiming));
    return MLGGD_OK;
}

// A stream of its own is only worth having if it does NOT share a hardware queue with the engine's main stream: the
// HIP runtime multiplexes streams onto a few hardware queues (by reference count, so the mapping depends on every
// stream the process has created and destroyed before), and two streams on one queue serialise.  Round 3, 1-rank
// rehearsal: the first communicator engine created after other engines had come and gone ran its step in 251 instead
// of 173 us for exactly that reason.  (Stream priorities are no way out: a high-priority communication stream made the
// first engine of a process run at 770 us per step.)  So the stream is PROBED: a 300 us spin kernel on the main stream,
// an empty kernel on the candidate; the candidate is kept if its kernel finishes while the spin is still running.
// Rejected candidates are destroyed only afterwards, so that each new one lands on another queue.
static int create_concurrent_stream(mlggd_engine *e, hipStream_t *out, const char *what) {
    hipEvent_t ev_main = nullptr, ev_cand = nullptr;
    HIPCHK(hipEventCreateWithFlags(&ev_main, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ev_cand, hipEventDisableTiming));
    std::vector<hipStream_t> rejected;
    hipStream_t keep = nullptr;
    int rc = MLGGD_OK, tries = 0;
    static const bool verbose = getenv("MLGGD_VERBOSE") != nullptr;
    for (; tries < 8 && !keep && rc == MLGGD_OK; tries++) {
        hipStream_t cand = nullptr;
        if (hipStreamCreateWithFlags(&cand, hipStreamNonBlocking) != hipSuccess) {
            rc = fail(MLGGD_ERR_DEVICE, "cannot create the %s stream", what);
            break;
        }
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, e->stream, 30000ll);  // 300 us of the 100 MHz wall clock
        hipEventRecord(ev_main, e->stream);
        hipLaunchKernelGGL(k_nop, dim3(1), dim3(64), 0, cand);
        hipEventRecord(ev_cand, cand);
        hipEventSynchronize(ev_cand);
        const bool concurrent = hipEventQuery(ev_main) == hipErrorNotReady;
        hipStreamSynchronize(e->stream);
        if (hipGetLastError() != hipSuccess) rc = fail(MLGGD_ERR_DEVICE, "probing the %s stream failed", what);
        if (concurrent) keep = cand;
        else rejected.push_back(cand);
    }
    if (!keep && !rejected.empty()) {  // no concurrent queue to be had: correct anyway, only slower
        keep = rejected.back();
        rejected.pop_back();
        fprintf(stderr, "mlggd: the %s stream shares a hardware queue with the main stream (no free queue after %d tries)\n",
                what, tries);
    } else if (verbose) {
        fprintf(stderr, "mlggd: %s stream found after %d candidate(s)\n", what, tries);
    }
    for (hipStream_t r : rejected) hipStreamDestroy(r);
    hipEventDestroy(ev_main);
    hipEventDestroy(ev_cand);
    *out = keep;
    return rc;
}
static int create_comm_stream(mlggd_engine *e) { return create_concurrent_stream(e, &e->comm_stream, "communication"); }

int mlggd_comm_unique_id(void *id) {
    if (!id) return fail(MLGGD_ERR_ARG, "id is NULL");
    CHK(rccl_load());
    RcclUniqueId uid;
    NCCLCHK(g_rccl.GetUniqueId(&uid));
    memcpy(id, &uid, sizeof(uid));
    return MLGGD_OK;
}

int mlggd_comm_init(mlggd_handle e, const void *id, int world_size, int rank) {
    if (!e || !id) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (world_size < 1 || rank < 0 || rank >= world_size)
        return fail(MLGGD_ERR_ARG, "rank %d / world_size %d invalid", rank, world_size);
    if (e->comm) return fail(MLGGD_ERR_STATE, "communicator already initialised");
    if (e->nat_frames > 0) return fail(MLGGD_ERR_STATE, "mlggd_comm_init: an engine with nat_frames = %d runs on a single device", e->nat_frames);
    if (e->opt_kind == MLGGD_OPT_ADAM) return fail(MLGGD_ERR_STATE, "mlggd_comm_init: an engine whose optimizer is Adam runs on a single device");
    if (e->cfg.dropoutflag == 1 && world_size > 1)
        return fail(MLGGD_ERR_ARG, "dropout is not supported on the data-parallel path");
    // the exchange mode first: a request the shape rules out must fail BEFORE a communicator exists (every rank takes
    // the same branch, so nobody is left waiting inside ncclCommInitRank)
    int mode;
    {
        const char *m = getenv("MLGGD_DP_MODE");  // "gather" | "shard" | "allreduce"; default: gather where usable,
        // sharded update from 6 ranks on (the W all-gather costs ~922/world us over world-1 links, the replicated
        // update ~35 us per extra rank: DESIGN.md section 6 -- a cost model, not yet a measurement)
        mode = gather_usable(e, world_size) ? (world_size >= 6 ? 2 : 1) : 0;
        if (m && !strcmp(m, "allreduce")) mode = 0;
        if (m && (!strcmp(m, "gather") || !strcmp(m, "shard") || !strcmp(m, "shard_a2a"))) {
            if (!gather_usable(e, world_size))
                return fail(MLGGD_ERR_ARG, "MLGGD_DP_MODE=%s needs bunchsize %% 32 == 0 and world*bunchsize in {64,128,256,512,1024}", m);
            mode = !strcmp(m, "gather") ? 1 : 2;
            e->dp_a2a = !strcmp(m, "shard_a2a") ? 1 : 0;  // opt-in only: no default or threshold changes before a scaling record exists
            if (e->dp_a2a && e->cfg.dropoutflag == 1)
                return fail(MLGGD_ERR_ARG, "MLGGD_DP_MODE=shard_a2a: dropout masks the row-major activations, which this mode keeps blocked by owner");
        }
    }
    CHK(rccl_load());
    HIPCHK(hipSetDevice(e->device));
    RcclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    NCCLCHK(g_rccl.CommInitRank(&e->comm, world_size, uid, rank));
    e->world = world_size;
    e->rank = rank;
    e->dp_mode = mode;
    dp_knobs(e);
    if (const char *v = getenv("MLGGD_DP_STAT_COMM"))
        if (atoi(v) != 0 && e->cfg.MLflag == 1) {
            if (!g_rccl.CommSplit) return fail(MLGGD_ERR_COMM, "MLGGD_DP_STAT_COMM=1: librccl has no ncclCommSplit");
            NCCLCHK(g_rccl.CommSplit(e->comm, 0, rank, &e->stat_comm, nullptr));  // collective: every rank takes this branch (same env, same MLflag)
        }
    CHK(create_comm_stream(e));
    if (e->dp_a2a && (!g_rccl.Send_ || !g_rccl.Recv_)) return fail(MLGGD_ERR_COMM, "MLGGD_DP_MODE=shard_a2a: librccl has no ncclSend / ncclRecv");
    if (e->dp_mode >= 1) {
        if (e->dp_a2a) CHK(shard_alloc(e));  // the block table first: the all-to-all buffers are sized by it
        CHK(gather_alloc(e));
        return (e->dp_mode == 2 && !e->dp_a2a) ? shard_alloc(e) : MLGGD_OK;
    }
    return allreduce_alloc(e);
}

// Test hook: emulate `world_size` ranks on ONE GPU, without a communicator.  Every training step then
// consumes one GLOBAL minibatch of world_size*bunchsize rows of the resident chunk; emulated rank r owns rows
// [r*bunchsize, (r+1)*bunchsize) of it (the partition of SURVEY 8e; different rows on every rank).  The ranks run
// one after the other (fake_world_prepass, then the real exchange path for the last one) with device copies /
// adds in place of the RCCL calls.  The result must equal the single-device step with bunchsize
// world_size*bunchsize on the same rows -- the data-parallel contract.
// mode: 0 = factor all-gather, replicated update; 1 = factor all-gather, sharded update; 2 = gradient all-reduce.
int mlggd_debug_fake_world(mlggd_handle e, int world_size, int mode) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (e->comm || e->fake_world) return fail(MLGGD_ERR_STATE, "communicator already initialised");
    if (e->nat_frames > 0) return fail(MLGGD_ERR_STATE, "mlggd_debug_fake_world: an engine with nat_frames = %d runs on a single device", e->nat_frames);
    if (e->opt_kind == MLGGD_OPT_ADAM) return fail(MLGGD_ERR_STATE, "mlggd_debug_fake_world: an engine whose optimizer is Adam runs on a single device");
    if (mode < 0 || mode > 3) return fail(MLGGD_ERR_ARG, "mode %d not in 0..3", mode);
    if (world_size < 1 || (mode != 2 && !gather_usable(e, world_size)))
        return fail(MLGGD_ERR_ARG, "fake world of %d ranks: needs bunchsize %% 32 == 0 and world*bunchsize in {64,...,1024}", world_size);
    if (e->cfg.dropoutflag == 1 && world_size > 1)
        return fail(MLGGD_ERR_ARG, "dropout is not supported on the data-parallel path");
    HIPCHK(hipSetDevice(e->device));
    e->world = world_size;
    e->rank = world_size - 1;  // the rank that takes the real exchange path; the others are emulated before it
    e->fake_world = true;
    e->dp_mode = mode == 2 ? 0 : (mode == 1 || mode == 3) ? 2 : 1;
    e->dp_a2a = mode == 3 ? 1 : 0;
    if (e->dp_a2a && e->cfg.dropoutflag == 1) return fail(MLGGD_ERR_ARG, "fake world: dropout is not supported with the all-to-all form");
    dp_knobs(e);
    CHK(create_comm_stream(e));
    CHK(dev_alloc(e, &e->colsum_tot, e->Dp));
    if (mode == 2) {
        CHK(allreduce_alloc(e));
        for (int l = 1; l < e->L; l++) CHK(dev_alloc(e, &e->Gpre[l], (size_t)e->lsp[l - 1] * e->lsp[l]));
        CHK(dev_alloc(e, &e->gbpre, e->gb_all_count));
        CHK(keep_alloc(e));
        HIPCHK(hipStreamSynchronize(e->stream));
        return MLGGD_OK;
    }
    if (mode == 3) CHK(shard_alloc(e));
    CHK(gather_alloc(e));
    if (mode == 1) CHK(shard_alloc(e));
    CHK(keep_alloc(e));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}
// size and rank of the RCCL communicator as RCCL itself reports them (ncclCommCount / ncclCommUserRank);
// 0 / -1 without a communicator
int mlggd_comm_info(mlggd_handle e, int *nranks, int *rank) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    int n = 0, r = -1;
    if (e->comm) {
        if (!g_rccl.CommCount || !g_rccl.CommUserRank) return fail(MLGGD_ERR_COMM, "librccl lacks ncclCommCount / ncclCommUserRank");
        NCCLCHK(g_rccl.CommCount(e->comm, &n));
        NCCLCHK(g_rccl.CommUserRank(e->comm, &r));
    }
    if (nranks) *nranks = n;
    if (rank) *rank = r;
    return MLGGD_OK;
}
// number of cached launch plans of the persistent dW kernel (tests: it must not grow with the step count)
int mlggd_debug_plan_count(mlggd_handle e, int *plans) {
    if (!e || !plans) return fail(MLGGD_ERR_ARG, "NULL argument");
    *plans = (int)e->dwp_tables.size();
    return MLGGD_OK;
}
// the engine's growable buffers (devbuf.h) and those of its live groups: device allocations they have made since the
// engine was created, and the bytes they hold now (tests: no call in the steady state allocates)
int mlggd_debug_buffers(mlggd_handle e, int64_t *allocations, int64_t *bytes) {
    if (!e || !allocations || !bytes) return fail(MLGGD_ERR_ARG, "NULL argument");
    *allocations = e->bufs.allocs;
    *bytes = e->bufs.bytes;
    return MLGGD_OK;
}
int mlggd_debug_gemm_plan(mlggd_handle e, int layer, int *fwd_waves, int *dx_waves) {
    if (!e || !fwd_waves || !dx_waves) return fail(MLGGD_ERR_ARG, "NULL argument");
    if (layer < 1 || layer >= e->L) return fail(MLGGD_ERR_ARG, "layer %d not in 1..%d", layer, e->L - 1);
    *fwd_waves = fwd64_used(e, layer) ? 1 : 4;  // (the output layer's 4 waves x out_slabs otherwise)
    *dx_waves = dx64_used(e, layer) ? 1 : 4;
    return MLGGD_OK;
}
int mlggd_debug_out_slabs(mlggd_handle e, int *slabs) {
    if (!e || !slabs) return fail(MLGGD_ERR_ARG, "NULL argument");
    *slabs = e->S_out;
    return MLGGD_OK;
}
int mlggd_get_activation(mlggd_handle e, int *act) {
    if (!e || !act) return fail(MLGGD_ERR_ARG, "NULL argument");
    *act = e->cfg.activation;
    return MLGGD_OK;
}
int mlggd_dp_mode(mlggd_handle e, int *mode) {
    if (!e || !mode) return fail(MLGGD_ERR_ARG, "NULL argument");
    // 0 single device, 1 all-reduce, 2 gather, 3 gather + sharded update, 4 = 3 with the activations by all-to-all
    *mode = (e->comm || e->fake_world) ? (e->dp_a2a ? 4 : 1 + e->dp_mode) : 0;
    return MLGGD_OK;
}

// Diagnostic: out[i] = fn(x[i], y) evaluated ON THE DEVICE with the same libm calls the kernels use
// ("powf" "expf" "sigmoid" "div"); tests measure their distance to the oracle's host libm in ulps.
int mlggd_debug_math(mlggd_handle e, const char *fn, const float *x, float y, float *out, size_t n) {
    if (!e || !fn || (n > 0 && (!x || !out))) return fail(MLGGD_ERR_ARG, "NULL argument");
    const int f = !strcmp(fn, "powf") ? 0 : !strcmp(fn, "expf") ? 1 : !strcmp(fn, "sigmoid") ? 2 : !strcmp(fn, "div") ? 3 : !strcmp(fn, "exp_det") ? 4 : !strcmp(fn, "pow_det") ? 5 : !strcmp(fn, "sigmoid4") ? 6 : !strcmp(fn, "relu") ? 7 : -1;
    if (f < 0) return fail(MLGGD_ERR_ARG, "unknown function '%s'", fn);
    if (n == 0) return MLGGD_OK;
    HIPCHK(hipSetDevice(e->device));
    DevBufs b;
    float *dx = nullptr, *dout = nullptr;
    CHK(b.alloc(&dx, n));
    CHK(b.alloc(&dout, n));
    if (hipMemcpyAsync(dx, x, n * sizeof(float), hipMemcpyHostToDevice, e->stream) != hipSuccess) return MLGGD_ERR_DEVICE;
    hipLaunchKernelGGL(k_debug_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, f, dx, y, dout, n);
    CHK(launch_check("k_debug_math"));
    if (hipMemcpyAsync(out, dout, n * sizeof(float), hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess)  // the buffers are freed on return
        return fail(MLGGD_ERR_DEVICE, "mlggd_debug_math: copy back failed");
    return MLGGD_OK;
}

// ---- per-kernel-class timing inside the timed region (bench.py roofline object)
int mlggd_profile_select(mlggd_handle e, const char *kernel_class, int layer, int max_launches) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    HIPCHK(hipSetDevice(e->device));
    e->prof_class = -1;
    e->prof_used = 0;
    if (!kernel_class || !*kernel_class) return MLGGD_OK;
    for (int c = 0; c < KC_COUNT; c++)
        if (!strcmp(kernel_class, kKernelClassName[c])) e->prof_class = c;
    if (e->prof_class < 0) return fail(MLGGD_ERR_ARG, "unknown kernel class '%s'", kernel_class);
    e->prof_layer = layer;
    if (max_launches < 1) max_launches = 1;
    e->prof_cap = 0;  // until the pool holds that many pairs
    while (e->prof_ev.size() < (size_t)2 * max_launches) {
        hipEvent_t ev;
        HIPCHK(hipEventCreate(&ev));
        e->prof_ev.push_back(ev);
    }
    e->prof_cap = (size_t)2 * max_launches;
    return MLGGD_OK;
}

int mlggd_profile_stride(mlggd_handle e, int every_nth_step) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    e->prof_stride = every_nth_step < 1 ? 1 : every_nth_step;
    return MLGGD_OK;
}

int mlggd_profile_read(mlggd_handle e, float *mean_usec, int *launches) {
    if (!e || !mean_usec) return fail(MLGGD_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    double tot = 0;
    int n = 0;
    for (size_t i = 0; i + 1 < e->prof_used; i += 2) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e->prof_ev[i], e->prof_ev[i + 1]));
        tot += ms;
        n++;
    }
    *mean_usec = n ? (float)(tot * 1000.0 / n) : 0.0f;
    if (launches) *launches = n;
    e->prof_used = 0;
    return MLGGD_OK;
}

// Diagnostic: phase stamps of the NEXT launch of (class, layer); see kernels.hip.h stamp().
int mlggd_debug_stamp_select(mlggd_handle e, const char *kernel_class, int layer) {
    if (!e || !kernel_class) return fail(MLGGD_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(e->stamp_buf.grow(8 * 8192, 8 * 8192, e->bufs, nullptr, nullptr));
    HIPCHK(hipMemsetAsync(e->stamp_buf.p, 0, e->stamp_buf.cap * sizeof(long long), e->stream));
    e->stamp_class = -1;
    for (int c = 0; c < KC_COUNT; c++)
        if (!strcmp(kernel_class, kKernelClassName[c])) e->stamp_class = c;
    if (e->stamp_class < 0) return fail(MLGGD_ERR_ARG, "unknown kernel class '%s'", kernel_class);
    e->stamp_layer = layer;
    e->stamp_blocks = 0;
    return MLGGD_OK;
}

int mlggd_debug_stamp_read(mlggd_handle e, long long *out, int cap_blocks, int *blocks) {
    if (!e || !out || !blocks) return fail(MLGGD_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int n = e->stamp_blocks < cap_blocks ? e->stamp_blocks : cap_blocks;
    if (n > 0) HIPCHK(hipMemcpy(out, e->stamp_buf.p, (size_t)n * 8 * sizeof(long long), hipMemcpyDeviceToHost));
    *blocks = n;
    return MLGGD_OK;
}

// Cost of one HIP-event bracket on the engine's stream, calibrated in-process: a kernel
// bracketed once measures overhead + t, bracketed twice back to back overhead + 2t, so
// overhead = 2*T1 - T2.  Uses an empty kernel (a kernel that writes memory would make the second of two
// back-to-back launches wait for the first one's dirty lines and skew T2).
int mlggd_profile_overhead(mlggd_handle e, float *usec) {
    if (!e || !usec) return fail(MLGGD_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(e->device));
    const int reps = 40;
    std::vector<hipEvent_t> ev(4 * reps);
    for (auto &x : ev) HIPCHK(hipEventCreate(&x));
    auto nop = [&]() -> int {
        hipLaunchKernelGGL(k_nop, dim3(256), dim3(256), 0, e->stream);
        return launch_check("k_nop");
    };
    for (int r = 0; r < reps; r++) {
        HIPCHK(hipEventRecord(ev[4 * r], e->stream));
        CHK(nop());
        HIPCHK(hipEventRecord(ev[4 * r + 1], e->stream));
        HIPCHK(hipEventRecord(ev[4 * r + 2], e->stream));
        CHK(nop());
        CHK(nop());
        HIPCHK(hipEventRecord(ev[4 * r + 3], e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    double t1 = 0, t2 = 0;
    for (int r = 4; r < reps; r++) {  // first reps warm up
        float a = 0, b = 0;
        HIPCHK(hipEventElapsedTime(&a, ev[4 * r], ev[4 * r + 1]));
        HIPCHK(hipEventElapsedTime(&b, ev[4 * r + 2], ev[4 * r + 3]));
        t1 += a;
        t2 += b;
    }
    for (auto &x : ev) hipEventDestroy(x);
    const double ov = (2 * t1 - t2) / (reps - 4) * 1000.0;
    *usec = ov > 0 ? (float)ov : 0.0f;
    return MLGGD_OK;
}

// Static description of the launch plan (DESIGN.md "kernels"): algorithmic FLOPs and bytes of
// one launch of the (class, layer) kernel; layer 0 = sum over layers.
int mlggd_dw_launches_per_step(mlggd_handle e, int *launches) {
    if (!e || !launches) return fail(MLGGD_ERR_ARG, "NULL argument");
    const bool dp = e->comm != nullptr || e->fake_world;
    const bool merged = (!dp && e->opt_kind != MLGGD_OPT_ADAM && e->dw_merge && dwp_usable(e)) || (dp && e->dp_mode >= 1);
    const bool fine = dp && e->dp_mode == 1 && e->dp_fine != 0 && e->L - 1 >= 2;
    *launches = fine ? 2 : merged ? 1 : e->L - 1;
    return MLGGD_OK;
}

int mlggd_kernel_work(mlggd_handle e, const char *kernel_class, int layer, double *flops, double *bytes) {
    if (!e || !kernel_class) return fail(MLGGD_ERR_ARG, "NULL argument");
    double f = 0, by = 0;
    // the gather path runs the dW kernel over the global minibatch on every rank
    // the gather paths run the dW kernel over the global minibatch: replicated (dp_mode 1) on all tiles,
    // sharded (dp_mode 2) on this rank's 1/world of the weight rows
    const bool dpx = (e->comm != nullptr || e->fake_world) && e->dp_mode >= 1 && !strcmp(kernel_class, "dw");
    const double W = e->world, B = e->B;
    // algorithmic figures: the multiply-adds of the GEMM and the tensors it reads and writes.  The activation epilogue
    // is not counted -- neither the sigmoid's exponential and division nor the rectifier's comparison -- so the
    // figures, and the roofline fractions built on them, are the same for both activations.
    auto gemm = [&](const char *cls, int l, double &ff, double &bb) {
        if (l < 1 || l >= e->L) return;
        const double K = e->ls[l - 1], N = e->ls[l];
        if (!strcmp(cls, "fwd")) {
            ff += 2.0 * B * K * N;
            bb += 4.0 * (K * N + B * K + 2 * B * N);
        } else if (!strcmp(cls, "dx")) {
            if (l == 1) return;
            ff += 2.0 * B * K * N;
            bb += 4.0 * (K * N + B * N + 3 * B * K);
        } else if (!strcmp(cls, "dw")) {
            if (!dpx) {
                ff += 2.0 * B * K * N;
                bb += 4.0 * (4 * K * N + B * K + B * N);  // W, delta read + written
            } else if (e->dp_mode == 1) {
                ff += 2.0 * B * W * K * N;
                bb += 4.0 * (4 * K * N + B * W * K + B * W * N);
            } else {
                ff += 2.0 * B * W * K * N / W;
                bb += 4.0 * (4 * K * N / W + B * W * K / W + B * W * N);
            }
        }
    };
    for (int l = 1; l < e->L; l++) {
        if (layer != 0 && layer != l) continue;
        gemm(kernel_class, l, f, by);
    }
    if (flops) *flops = f;
    if (bytes) *bytes = by;
    return MLGGD_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ spectral front end / back end (spectral.hip.h)
// Wav2LPS_be / LPS2Wav_be / decode.m of the original project.  The window and twiddle tables are computed in double,
// rounded to float and uploaded once per (device, rate).
namespace {

struct SpecPlan {
    SpecDims d;
    float *win = nullptr;    // [L], mirrored half table
    float2 *tw = nullptr;    // [M/2] exp(-2 pi i j / M)
    float2 *tws = nullptr;   // [D]   exp(-2 pi i k / N)
};
constexpr int SPEC_MAX_DEVICES = 64;
std::mutex g_spec_mu;
SpecPlan g_spec[SPEC_MAX_DEVICES][3];

// floor of the power spectrum before its log, and of exp(lps) on the way back
const float kSpecFloor = (float)exp(-50.0);

int spec_dims(int fs_khz, SpecDims *d, int *slot = nullptr) {
    if (!spec_rule::rate(fs_khz, d, slot)) return fail(MLGGD_ERR_ARG, "fs_khz %d: must be 8, 11 or 16", fs_khz);
    return MLGGD_OK;
}

// twiddle in double, an exact 0 where the value is 0 (the DC / Nyquist outputs stay real)
float2 twiddle(int k, int n) {
    const double a = -2.0 * M_PI * k / n;
    double c = cos(a), s = sin(a);
    if (4 * k == n || 4 * k == 3 * n) c = 0.0;
    if (2 * k == n || k == 0) s = 0.0;
    return make_float2((float)c, (float)s);
}

// a table of a process-lifetime plan: allocated on the current device and filled by a blocking copy
template <typename T>
int upload_table(const std::vector<T> &h, T **out) {
    T *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, h.size() * sizeof(T)));
    HIPCHK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = d;
    return MLGGD_OK;
}

// the plan of (current device, rate); the caller has selected the device
int spec_plan(int device, int fs_khz, const SpecPlan **out) {
    SpecDims d;
    int slot;
    CHK(spec_dims(fs_khz, &d, &slot));
    if (device < 0 || device >= SPEC_MAX_DEVICES) return fail(MLGGD_ERR_ARG, "device %d out of range", device);
    std::lock_guard<std::mutex> lock(g_spec_mu);
    SpecPlan &p = g_spec[device][slot];
    if (!p.win) {
        std::vector<float> win(d.L);
        for (int i = 0; i < d.L / 2; i++) win[i] = (float)(0.54 - 0.46 * cos(2.0 * M_PI * i / (d.L - 1)));  // FEfunc.c
        for (int i = d.L / 2; i < d.L; i++) win[i] = win[d.L - 1 - i];
        std::vector<float2> tw(d.M / 2), tws(d.D);
        for (int j = 0; j < d.M / 2; j++) tw[j] = twiddle(j, d.M);
        for (int k = 0; k < d.D; k++) tws[k] = twiddle(k, d.N);
        float *w = nullptr;
        float2 *a = nullptr, *b = nullptr;
        CHK(upload_table(win, &w));
        CHK(upload_table(tw, &a));
        CHK(upload_table(tws, &b));
        p.d = d, p.win = w, p.tw = a, p.tws = b;
    }
    *out = &p;
    return MLGGD_OK;
}

// ... after making that device the current one
int spec_plan_on(int device, int fs_khz, const SpecPlan **out) {
    HIPCHK(hipSetDevice(device));
    return spec_plan(device, fs_khz, out);
}

unsigned spec_grid(int frames) { return (unsigned)((frames + SPEC_FRAMES - 1) / SPEC_FRAMES); }

int launch_analysis(const SpecPlan *p, const int16_t *wave, int F, float *lps, float2 *X, hipStream_t st) {
    if (F == 0) return MLGGD_OK;
    hipLaunchKernelGGL(k_lps_analysis, dim3(spec_grid(F)), dim3(64 * SPEC_FRAMES), 0, st, wave, F, p->d, p->win, p->tw,
                       p->tws, kSpecFloor, lps, X);
    return launch_check("k_lps_analysis");
}

// the same over FT >= 1 packed frames of n utterances that all have frames: wave_off / frame_off [n + 1] and utt_of
// [FT] (or NULL: the kernel searches frame_off) are on the device; lps or X may be NULL
int launch_analysis_seg(const SpecPlan *p, const int16_t *wave, const long long *wave_off, const int *frame_off,
                        const int *utt_of, int n, int FT, float *lps, float2 *X, hipStream_t st) {
    hipLaunchKernelGGL(k_lps_analysis_seg, dim3(spec_grid(FT)), dim3(64 * SPEC_FRAMES), 0, st, wave, wave_off, frame_off,
                       utt_of, n, FT, p->d, p->win, p->tw, p->tws, kSpecFloor, lps, X);
    return launch_check("k_lps_analysis_seg");
}

// eta (optional, with mean): the equalisation factors of gv_rule.h; without them the launch is the one it always was
int launch_synthesis(const SpecPlan *p, const float *src, const float *mean, const float *inv, const float2 *X, int t0,
                     int nf, float *blk, hipStream_t st, float *lps_den = nullptr, const float *eta = nullptr,
                     const MaskArgs *mk = nullptr) {
    if (nf == 0) return MLGGD_OK;
    if (mk) {  // a mask engine: src rows of 2 D outputs, post-filtered against the noisy rows (mask_rule.h)
        if (eta) {
            hipLaunchKernelGGL(k_lps_synthesis_mask_gv, dim3(spec_grid(nf)), dim3(64 * SPEC_FRAMES), 0, st, src, mean, inv,
                               eta, X, t0, nf, p->d, p->win, p->tw, p->tws, kSpecFloor, blk, lps_den, *mk);
            return launch_check("k_lps_synthesis_mask_gv");
        }
        hipLaunchKernelGGL(k_lps_synthesis_mask, dim3(spec_grid(nf)), dim3(64 * SPEC_FRAMES), 0, st, src, mean, inv, X, t0,
                           nf, p->d, p->win, p->tw, p->tws, kSpecFloor, blk, lps_den, *mk);
        return launch_check("k_lps_synthesis_mask");
    }
    if (eta) {
        hipLaunchKernelGGL(k_lps_synthesis_gv, dim3(spec_grid(nf)), dim3(64 * SPEC_FRAMES), 0, st, src, mean, inv, eta, X,
                           t0, nf, p->d, p->win, p->tw, p->tws, kSpecFloor, blk, lps_den);
        return launch_check("k_lps_synthesis_gv");
    }
    hipLaunchKernelGGL(k_lps_synthesis, dim3(spec_grid(nf)), dim3(64 * SPEC_FRAMES), 0, st, src, mean, inv, X, t0, nf,
                       p->d, p->win, p->tw, p->tws, kSpecFloor, blk, lps_den);
    return launch_check("k_lps_synthesis");
}

int launch_ola(const SpecPlan *p, const float *blk, int F, float *out_f, int16_t *out_i, hipStream_t st) {
    const int n_out = (int)spec_rule::out_samples(p->d, F);
    hipLaunchKernelGGL(k_ola, dim3((n_out + 255) / 256), dim3(256), 0, st, blk, F, p->d, p->win, out_f, out_i, n_out);
    return launch_check("k_ola");
}

// out (int16) and out_f32 (optional) of n_out samples from the time blocks of F frames
int ola_to_host(const SpecPlan *p, const float *blk, int F, int16_t *out, float *out_f32, hipStream_t st) {
    const size_t n_out = (size_t)spec_rule::out_samples(p->d, F);
    DevBufs b;
    float *of = nullptr;
    int16_t *oi = nullptr;
    CHK(b.alloc(&oi, n_out));
    if (out_f32) CHK(b.alloc(&of, n_out));
    CHK(launch_ola(p, blk, F, of, oi, st));
    if (out) HIPCHK(hipMemcpyAsync(out, oi, n_out * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    if (out_f32) HIPCHK(hipMemcpyAsync(out_f32, of, n_out * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MLGGD_OK;
}

int launch_nat_estimate(const mlggd_engine *e, const float *rows, const int *d_frame_off, int n_utts, int D,
                        const float *mean, const float *inv, float *out) {
    const size_t work = (size_t)n_utts * D;
    hipLaunchKernelGGL(k_nat_estimate, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, e->stream, rows, d_frame_off,
                       n_utts, D, e->nat_frames, mean, inv, out);
    return launch_check("k_nat_estimate");
}

// What a wave entry asks of its engine: the rate exists (*d receives its dimensions), fea_context is odd (decoding: a
// frame sits in the middle of its window) or at least 1 (loading), fea_context frames of D bins, plus the noise row on
// a NAT engine, fill layer 0 and the net puts out one frame of D bins.
int check_wave_engine(const mlggd_engine *e, int fs_khz, int ctx, bool decoding, SpecDims *d) {
    CHK(spec_dims(fs_khz, d));
    if (decoding && (ctx < 1 || ctx % 2 == 0)) return fail(MLGGD_ERR_ARG, "fea_context %d must be odd", ctx);
    if (ctx < 1) return fail(MLGGD_ERR_ARG, "fea_context %d < 1", ctx);
    // a mask engine puts out the frame's D bins twice, LPS then mask: the rate must be the one it was created for
    if (e->mask_bins && e->mask_bins != d->D)
        return fail(MLGGD_ERR_ARG, "mask_bins %d != %d bins at %d kHz", e->mask_bins, d->D, fs_khz);
    if (e->nat_frames > 0 && ((long long)ctx + 1) * d->D != e->K0)
        return fail(MLGGD_ERR_ARG, "(fea_context %d + 1) x %d bins != layersizes[0] = %d (nat_frames = %d)", ctx, d->D,
                    e->K0, e->nat_frames);
    if (e->nat_frames == 0 && (long long)ctx * d->D != e->K0)
        return fail(MLGGD_ERR_ARG, "fea_context %d x %d bins != layersizes[0] = %d", ctx, d->D, e->K0);
    if (e->mask_bins) return MLGGD_OK;  // its last layer is 2 mask_bins wide (mlggd_create)
    if (e->D != d->D) return fail(MLGGD_ERR_ARG, "output dimension %d != %d bins at %d kHz", e->D, d->D, fs_khz);
    return MLGGD_OK;
}

// ... and that it stands alone.  The decode entries take an engine that has joined a communicator of one rank; the
// loaders and live groups (no_comm) take none that has joined any.
int check_single_device(const mlggd_engine *e, const char *who, bool no_comm) {
    if ((no_comm && e->comm) || e->world > 1 || e->fake_world)
        return fail(MLGGD_ERR_STATE, "%s runs on a single-device engine", who);
    return MLGGD_OK;
}

// One decode chunk: n output frames read through windows of ctx rows over a stream of `rows` rows.  The idle raw set is
// borrowed, fill(set) writes its stream and first_frame (and nat_row on a NAT engine, whose samples then read the
// noise table `nat`), the set becomes current, the net runs and its n rows are resynthesised against X into blk from
// frame t0 on (lps_den: the de-normalised rows, optional; eta: the equalisation factors in effect, or nullptr).  The
// set is marked in use until that has run.
// the factors a decode call or push applies: those of mlggd_set_gv while they are on
const float *gv_factors(const mlggd_engine *e) { return e->gv_on ? e->gv_dev.p : nullptr; }

// noisy_lps: the analysis' un-normalised rows of the whole call, indexed like X by the packed frame; read on a mask
// engine only, whose post-filter chooses between them and the estimate
template <typename Fill>
int decode_chunk(mlggd_engine *e, const SpecPlan *p, int rows, int n, int ctx, const Fill &fill, const float *nat,
                 const float *mean, const float *inv, const float *eta, const float2 *X, int t0, float *blk,
                 float *lps_den, const float *noisy_lps) {
    mlggd_engine::RawSet *r;
    CHK(raw_set_acquire(e, rows, n, ctx, 0, false, &r));
    CHK(fill(r));
    raw_set_commit(e, rows, n, ctx, 0);
    if (e->nat_frames) e->nat = nat;
    CHK(forward_resident(e, n));
    if (e->mask_bins) {
        const MaskArgs mk = {noisy_lps, e->mask_lo, e->mask_hi, e->mask_scale, e->mask_mode};
        CHK(launch_synthesis(p, e->chunk_out.p, mean, inv, X, t0, n, blk, e->stream, lps_den, eta, &mk));
    } else {
        CHK(launch_synthesis(p, e->chunk_out.p, mean, inv, X, t0, n, blk, e->stream, lps_den, eta));
    }
    HIPCHK(hipEventRecord(e->raw[e->raw_cur].last_use, e->stream));
    return MLGGD_OK;
}

// the frame stream of output frames [a, a + n) of an F-frame utterance, written by k_lps_stream (first_frame[i] = i)
// into the set r; on a NAT engine every sample takes row 0 of the noise table, the one noise row of the utterance
int load_frames_device(mlggd_engine *e, mlggd_engine::RawSet *r, const float *lps, int F, int a, int n, int ctx,
                       const float *mean, const float *inv) {
    const int fdim = stream_fdim(e, ctx), rows = n + ctx - 1;
    const size_t work = std::max((size_t)rows * fdim, (size_t)n);
    hipLaunchKernelGGL(k_lps_stream, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, e->stream, lps, F, fdim, a,
                       rows, (ctx - 1) / 2, mean, inv, r->feat.p, r->first.p, n);
    CHK(launch_check("k_lps_stream"));
    if (e->nat_frames) HIPCHK(hipMemsetAsync(r->nat_row.p, 0, (size_t)n * sizeof(int), e->stream));
    return MLGGD_OK;
}

// a workspace buffer as `count` elements of T (devbuf_rule::ws_bytes when it has to grow); the old contents are dropped
template <typename T>
int ws_grow(mlggd_engine *e, mlggd_engine::WsBuf &b, size_t count, T **out) {
    const size_t bytes = (count ? count : 1) * sizeof(T);
    HIPCHK(b.grow(bytes, devbuf_rule::ws_bytes(bytes), e->bufs, nullptr, &e->stream));
    *out = (T *)b.p;
    return MLGGD_OK;
}

// the quality report (score.hip.h) of FT packed frames: clean wave, LPS rows and noisy spectrum X on the device ->
// scores [2 n_utts] = segsnr, lsd.  Xc [FT][D] and fstat [3 FT] are scratch; sframes / utt_of may be NULL.
int launch_score(const SpecPlan *p, const int16_t *clean, const long long *wave_off, const int *frame_off,
                 const int *utt_of, const int *sframes, int n_utts, int FT, const float *lps, const float2 *X,
                 float2 *Xc, float *fstat, float *scores, hipStream_t st) {
    float *snr = fstat, *maxc = fstat + FT, *maxd = fstat + (size_t)2 * FT;
    hipLaunchKernelGGL(k_score_frames, dim3(spec_grid(FT)), dim3(64 * SPEC_FRAMES), 0, st, clean, wave_off, frame_off,
                       utt_of, sframes, n_utts, FT, p->d, p->win, p->tw, p->tws, kSpecFloor, kSpecFloor,
                       lps, X, Xc, snr, maxc, maxd);
    CHK(launch_check("k_score_frames"));
    hipLaunchKernelGGL(k_score_utt, dim3((unsigned)n_utts), dim3(64 * SCORE_UTT_WAVES), 0, st, frame_off, sframes,
                       p->d.D, kSpecFloor, lps, (const float2 *)Xc, (const float *)snr, (const float *)maxc,
                       (const float *)maxd, scores, scores + n_utts);
    return launch_check("k_score_utt");
}

// ---- STOI (stoi.hip.h, stoi_rule.h).  The window and the three resampling filters are computed in double, rounded to
// float and uploaded once per device; the FFT twiddles are the 16 kHz tables of the spectral plan (N = 512).
struct StoiPlan {
    float *win = nullptr;                       // [256]
    float *h[3] = {nullptr, nullptr, nullptr};  // [2 Lh + 1] per rate slot
};
StoiPlan g_stoi[SPEC_MAX_DEVICES];

int stoi_plan(int device, const StoiPlan **out, const SpecPlan **fft) {
    CHK(spec_plan(device, 16, fft));  // checks the device index too
    std::lock_guard<std::mutex> lock(g_spec_mu);
    StoiPlan &p = g_stoi[device];
    if (!p.win) {
        const int rates[3] = {8, 11, 16};
        for (int r : rates) {
            int pp, qq, slot;
            stoi_rule::rate(r, &pp, &qq, &slot);
            CHK(upload_table(stoi_rule::filter(pp, qq), &p.h[slot]));
        }
        float *dw = nullptr;
        CHK(upload_table(stoi_rule::window(), &dw));
        p.win = dw;
    }
    *out = &p;
    return MLGGD_OK;
}

// what the kernels need to know about a batch, found on the host before any device call
struct StoiJob {
    int p = 0, q = 0, slot = 0, FT = 0;
    long long T10 = 0;
};

// utt[u] for clean samples from coff[u] and processed samples from poff[u]: stoi_samples[u] (NULL: all) must lie in
// 0..len[u]; at most have[u] of them are scored (the processed wave may be shorter than the utterance)
int stoi_job(int fs_khz, int n_utts, const long long *coff, const long long *poff, const long long *len,
             const long long *have, const int64_t *stoi_samples, std::vector<StoiUtt> &utt, StoiJob *job) {
    if (!stoi_rule::rate(fs_khz, &job->p, &job->q, &job->slot))
        return fail(MLGGD_ERR_ARG, "fs_khz %d: must be 8, 11 or 16", fs_khz);
    utt.resize((size_t)n_utts);
    long long t10 = 0, ft = 0;
    for (int u = 0; u < n_utts; u++) {
        long long n = len[u];
        if (stoi_samples) {
            if (stoi_samples[u] < 0 || stoi_samples[u] > len[u])
                return fail(MLGGD_ERR_ARG, "utterance %d: stoi_samples %lld is outside 0..%lld, its samples", u,
                            (long long)stoi_samples[u], len[u]);
            n = stoi_samples[u];
        }
        if (n > have[u]) n = have[u];
        if (n > stoi_rule::kMaxSamples)
            return fail(MLGGD_ERR_ARG, "utterance %d: %lld samples exceed the %lld one wave may have", u, n,
                        (long long)stoi_rule::kMaxSamples);
        StoiUtt &U = utt[u];
        U.coff = coff[u], U.poff = poff[u], U.off10 = t10;
        U.len = (int)n;
        U.len10 = (int)stoi_rule::len10(n, job->p, job->q);
        U.foff = (int)ft;
        U.frames = (int)stoi_rule::frames(U.len10);
        t10 += U.len10;
        ft += U.frames;
        if (ft > INT32_MAX / 2)
            return fail(MLGGD_ERR_ARG, "the batch has more than %d STOI frames (reached at utterance %d)", INT32_MAX / 2, u);
    }
    job->T10 = t10, job->FT = (int)ft;
    return MLGGD_OK;
}

// device buffers of one STOI pass: utt [n], x [2 T10] (clean, processed at 10 kHz), f [31 FT] (frame energies, X and Y
// band roots), i [FT + n] (kept map, kept counts), res [2 n] (stoi; segment counts as int)
struct StoiDev {
    StoiUtt *utt;
    float *x, *f;
    int *i;
    float *res;
};

int launch_stoi(const StoiPlan *sp, const SpecPlan *fft, const StoiJob &job, const int16_t *clean, const int16_t *proc,
                int n_utts, const StoiDev &b, hipStream_t st) {
    const size_t T10 = (size_t)job.T10, FT = (size_t)job.FT;
    float *xc = b.x, *xp = b.x + T10, *en = b.f, *Xb = b.f + FT, *Yb = b.f + FT + FT * STOI_BANDS;
    int *map = b.i, *kept = b.i + FT;
    if (T10) {
        hipLaunchKernelGGL(k_stoi_resample, dim3((unsigned)((T10 + 255) / 256)), dim3(256), 0, st, clean, proc,
                           (const StoiUtt *)b.utt, n_utts, (const float *)sp->h[job.slot], job.p, job.q,
                           stoi_rule::half_taps(job.p, job.q), (long long)job.T10, xc, xp);
        CHK(launch_check("k_stoi_resample"));
    }
    if (FT) {
        hipLaunchKernelGGL(k_stoi_energy, dim3((unsigned)((FT + 3) / 4)), dim3(256), 0, st, (const float *)xc,
                           (const StoiUtt *)b.utt, n_utts, job.FT, (const float *)sp->win, en);
        CHK(launch_check("k_stoi_energy"));
    }
    hipLaunchKernelGGL(k_stoi_select, dim3((unsigned)n_utts), dim3(64 * STOI_SELECT_WAVES), 0, st,
                       (const StoiUtt *)b.utt, (const float *)en, map, kept);
    CHK(launch_check("k_stoi_select"));
    if (FT) {
        StoiBandTable bands;
        for (int j = 0; j < STOI_BANDS; j++) bands.lo[j] = stoi_rule::kBandLo[j], bands.hi[j] = stoi_rule::kBandHi[j];
        hipLaunchKernelGGL(k_stoi_bands, dim3(spec_grid(job.FT)), dim3(64 * SPEC_FRAMES), 0, st, (const float *)xc,
                           (const float *)xp, (const StoiUtt *)b.utt, n_utts, job.FT, (const float *)sp->win,
                           (const float2 *)fft->tw, (const float2 *)fft->tws, (const int *)map, (const int *)kept, bands,
                           Xb, Yb);
        CHK(launch_check("k_stoi_bands"));
    }
    hipLaunchKernelGGL(k_stoi_utt, dim3((unsigned)n_utts), dim3(64 * SCORE_UTT_WAVES), 0, st, (const StoiUtt *)b.utt,
                       (const int *)kept, (const float *)Xb, (const float *)Yb, (float)pow(10.0, 15.0 / 20.0), b.res,
                       (int *)(b.res + n_utts));
    return launch_check("k_stoi_utt");
}

void stoi_results(const float *h, int n_utts, float *stoi, int32_t *segments) {
    memcpy(stoi, h, (size_t)n_utts * sizeof(float));
    if (segments) memcpy(segments, h + n_utts, (size_t)n_utts * sizeof(int32_t));
}

}  // namespace

extern "C" {

int mlggd_wave_to_lps(int device, int fs_khz, int n_samples, const int16_t *wave, int *n_frames, float *lps) {
    SpecDims d;
    CHK(spec_dims(fs_khz, &d));
    if (n_samples < 0) return fail(MLGGD_ERR_ARG, "n_samples %d < 0", n_samples);
    if (!n_frames) return fail(MLGGD_ERR_ARG, "n_frames is NULL");
    const int F = (int)spec_rule::frames(d, n_samples);
    *n_frames = F;
    if (!lps || F == 0) return MLGGD_OK;
    if (!wave) return fail(MLGGD_ERR_ARG, "wave is NULL");
    const SpecPlan *p;
    CHK(spec_plan_on(device, fs_khz, &p));
    DevBufs b;
    int16_t *dw = nullptr;
    float *dl = nullptr;
    CHK(b.upload(&dw, wave, (size_t)spec_rule::out_samples(d, F)));  // the samples the frames cover
    CHK(b.alloc(&dl, (size_t)F * d.D));
    CHK(launch_analysis(p, dw, F, dl, nullptr, nullptr));
    HIPCHK(hipMemcpy(lps, dl, (size_t)F * d.D * sizeof(float), hipMemcpyDeviceToHost));
    return MLGGD_OK;
}

int mlggd_lps_to_wave(int device, int fs_khz, int n_samples, const int16_t *noisy, int n_frames, const float *lps,
                      int16_t *out, float *out_f32) {
    SpecDims d;
    CHK(spec_dims(fs_khz, &d));
    if (n_samples < d.L) return fail(MLGGD_ERR_ARG, "n_samples %d is shorter than one frame (%d)", n_samples, d.L);
    const int F = (int)spec_rule::frames(d, n_samples);
    if (n_frames != F)
        return fail(MLGGD_ERR_ARG, "n_frames %d: the %d noisy samples give %d frames", n_frames, n_samples, F);
    if (!noisy || !lps || !out) return fail(MLGGD_ERR_ARG, "noisy/lps/out is NULL");
    const SpecPlan *p;
    CHK(spec_plan_on(device, fs_khz, &p));
    DevBufs b;
    int16_t *dw = nullptr;
    float *dl = nullptr, *blk = nullptr;
    float2 *X = nullptr;
    CHK(b.upload(&dw, noisy, (size_t)spec_rule::out_samples(d, F)));
    CHK(b.upload(&dl, lps, (size_t)F * d.D));
    CHK(b.alloc(&X, (size_t)F * d.D));
    CHK(b.alloc(&blk, (size_t)F * d.L));
    CHK(launch_analysis(p, dw, F, nullptr, X, nullptr));
    CHK(launch_synthesis(p, dl, nullptr, nullptr, X, 0, F, blk, nullptr));
    return ola_to_host(p, blk, F, out, out_f32, nullptr);
}

int mlggd_enhance_wave(mlggd_handle e, int fs_khz, int fea_context, const float *norm_mean, const float *norm_inv_std,
                       int n_samples, const int16_t *noisy, int16_t *out, float *out_f32, int *n_out) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    SpecDims d;
    CHK(check_wave_engine(e, fs_khz, fea_context, true, &d));
    CHK(check_single_device(e, "mlggd_enhance_wave", false));
    if (n_samples < d.L) return fail(MLGGD_ERR_ARG, "n_samples %d is shorter than one frame (%d)", n_samples, d.L);
    if (!noisy || !norm_mean || !norm_inv_std || !out) return fail(MLGGD_ERR_ARG, "noisy/norm/out is NULL");
    const int F = (int)spec_rule::frames(d, n_samples);
    const size_t used = (size_t)spec_rule::out_samples(d, F);
    if (n_out) *n_out = (int)used;
    const SpecPlan *p;
    CHK(spec_plan_on(e->device, fs_khz, &p));
    hipStream_t st = e->stream;
    DevBufs b;
    int16_t *dw = nullptr;
    float *dl = nullptr, *blk = nullptr, *mean = nullptr, *inv = nullptr;
    float2 *X = nullptr;
    CHK(b.alloc(&dw, used));
    CHK(b.alloc(&dl, (size_t)F * d.D));
    CHK(b.alloc(&X, (size_t)F * d.D));
    CHK(b.alloc(&blk, (size_t)F * d.L));
    CHK(b.alloc(&mean, d.D));
    CHK(b.alloc(&inv, d.D));
    HIPCHK(hipMemcpyAsync(dw, noisy, used * sizeof(int16_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(mean, norm_mean, d.D * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(inv, norm_inv_std, d.D * sizeof(float), hipMemcpyHostToDevice, st));
    CHK(launch_analysis(p, dw, F, dl, X, st));  // the noisy wave is transformed once
    float *natz = nullptr;
    const int h_foff[2] = {0, F};
    if (e->nat_frames) {  // the utterance's noise row, once, from the analysed rows
        int *d_foff = nullptr;
        CHK(b.alloc(&natz, d.D));
        CHK(b.alloc(&d_foff, 2));
        HIPCHK(hipMemcpyAsync(d_foff, h_foff, sizeof(h_foff), hipMemcpyHostToDevice, st));
        CHK(launch_nat_estimate(e, dl, d_foff, 1, d.D, mean, inv, natz));
    }
    // chunks of at most the chunk capacity; each one's stream carries (ctx - 1) / 2 context frames on either side,
    // so consecutive streams overlap by ctx - 1 frames and every output frame sees the same input rows
    const int cap = chunk_cap(e);
    for (int a = 0; a < F; a += cap) {
        const int n = std::min(cap, F - a);
        auto fill = [&](mlggd_engine::RawSet *r) { return load_frames_device(e, r, dl, F, a, n, fea_context, mean, inv); };
        CHK(decode_chunk(e, p, n + fea_context - 1, n, fea_context, fill, natz, mean, inv, gv_factors(e), X, a, blk, nullptr, dl));
    }
    return ola_to_host(p, blk, F, out, out_f32, st);
}

int mlggd_enhance_waves_layout(int fs_khz, int n_utts, const int64_t *offsets, int32_t *frame_off, int64_t *out_off) {
    SpecDims d;
    CHK(spec_dims(fs_khz, &d));
    std::vector<long long> oo(out_off ? (size_t)std::max(n_utts, 0) + 1 : 0);  // the rule's tables are the device's types
    RULE(spec_rule::layout(d, n_utts, offsets, spec_rule::kShortFails, frame_off, out_off ? oo.data() : nullptr, nullptr,
                           RULE_MSG));
    std::copy(oo.begin(), oo.end(), out_off);
    return MLGGD_OK;
}

// mlggd_enhance_waves, and with clean != NULL mlggd_enhance_waves_scored (`who` names the entry point): the report is
// formed after the last chunk from the buffers of the pass (X, the de-normalised rows) and changes none of them
static int enhance_waves_run(mlggd_handle e, const char *who, int fs_khz, int fea_context, const float *norm_mean,
                             const float *norm_inv_std, int n_utts, const int16_t *noisy, const int16_t *clean,
                             const int64_t *offsets, const int32_t *score_frames, int16_t *out, float *out_f32,
                             float *lps_out, float *segsnr, float *lsd, const int64_t *stoi_samples = nullptr,
                             float *stoi = nullptr, int32_t *segments = nullptr) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    SpecDims d;
    CHK(check_wave_engine(e, fs_khz, fea_context, true, &d));
    CHK(check_single_device(e, who, false));
    if (n_utts < 0) return fail(MLGGD_ERR_ARG, "n_utts %d < 0", n_utts);
    if (n_utts == 0) return MLGGD_OK;
    if (!noisy || !offsets || !norm_mean || !norm_inv_std || !out)
        return fail(MLGGD_ERR_ARG, "noisy/offsets/norm/out is NULL");
    mlggd_engine::WavesWs &w = e->ww;
    w.h_frame_off.resize((size_t)n_utts + 1);
    w.h_out_off.resize((size_t)n_utts + 1);
    w.h_wave_off.resize((size_t)n_utts + 1);
    RULE(spec_rule::layout(d, n_utts, offsets, spec_rule::kShortFails, w.h_frame_off.data(), w.h_out_off.data(),
                           w.h_wave_off.data(), RULE_MSG));
    if (clean) RULE(spec_rule::check_score_frames(n_utts, w.h_frame_off.data(), score_frames, RULE_MSG));
    StoiJob sjob;
    if (stoi) {  // the enhanced wave of utterance u has out_off[u + 1] - out_off[u] samples: no more can be scored
        std::vector<long long> len((size_t)n_utts), have((size_t)n_utts);
        for (int u = 0; u < n_utts; u++) {
            len[u] = w.h_wave_off[u + 1] - w.h_wave_off[u];
            have[u] = w.h_out_off[u + 1] - w.h_out_off[u];
        }
        CHK(stoi_job(fs_khz, n_utts, w.h_wave_off.data(), w.h_out_off.data(), len.data(), have.data(), stoi_samples,
                     w.h_stoi_utt, &sjob));
    }
    const int FT = w.h_frame_off[n_utts];  // every utterance has a frame: FT >= n_utts
    const size_t n_wave = (size_t)w.h_wave_off[n_utts], n_out = (size_t)w.h_out_off[n_utts];
    const int cap = chunk_cap(e);
    // the stream rows of a chunk: its frames + (ctx - 1) per utterance it touches, in int
    if ((long long)std::min(cap, FT) + (long long)std::min(n_utts, cap) * (fea_context - 1) > INT32_MAX / 2)
        return fail(MLGGD_ERR_ARG, "a chunk of %d frames over %d utterances is too large", std::min(cap, FT), n_utts);
    const SpecPlan *p;
    CHK(spec_plan_on(e->device, fs_khz, &p));
    hipStream_t st = e->stream;
    int16_t *dw = nullptr, *oi = nullptr;
    float *dl = nullptr, *blk = nullptr, *of = nullptr, *den = nullptr, *norm = nullptr;
    float2 *X = nullptr;
    int *d_foff = nullptr, *d_utt = nullptr;
    long long *d_ooff = nullptr, *d_woff = nullptr;
    CHK(ws_grow(e, w.wave, n_wave, &dw));
    CHK(ws_grow(e, w.lps, (size_t)FT * d.D, &dl));
    CHK(ws_grow(e, w.X, (size_t)FT * d.D, &X));
    CHK(ws_grow(e, w.blk, (size_t)FT * d.L, &blk));
    CHK(ws_grow(e, w.out_i, n_out, &oi));
    if (out_f32) CHK(ws_grow(e, w.out_f, n_out, &of));
    if (lps_out || clean) CHK(ws_grow(e, w.lps_den, (size_t)FT * d.D, &den));
    int16_t *d_clean = nullptr;
    float2 *Xc = nullptr;
    float *fstat = nullptr, *scores = nullptr;
    int *d_sf = nullptr;
    if (clean) {
        CHK(ws_grow(e, w.clean, n_wave, &d_clean));
        CHK(ws_grow(e, w.Xc, (size_t)FT * d.D, &Xc));
        CHK(ws_grow(e, w.fstat, (size_t)3 * FT, &fstat));
        CHK(ws_grow(e, w.scores, (size_t)2 * n_utts, &scores));
        if (score_frames) CHK(ws_grow(e, w.sframes, (size_t)n_utts, &d_sf));
    }
    const StoiPlan *splan = nullptr;
    const SpecPlan *sfft = nullptr;
    StoiDev sdev = {};
    if (stoi) {
        CHK(stoi_plan(e->device, &splan, &sfft));
        CHK(ws_grow(e, w.stoi_utt, (size_t)n_utts, &sdev.utt));
        CHK(ws_grow(e, w.stoi_x, (size_t)2 * sjob.T10, &sdev.x));
        CHK(ws_grow(e, w.stoi_f, (size_t)(1 + 2 * STOI_BANDS) * sjob.FT, &sdev.f));
        CHK(ws_grow(e, w.stoi_i, (size_t)sjob.FT + n_utts, &sdev.i));
        CHK(ws_grow(e, w.stoi_res, (size_t)2 * n_utts, &sdev.res));
    }
    CHK(ws_grow(e, w.frame_off, (size_t)n_utts + 1, &d_foff));
    CHK(ws_grow(e, w.out_off, (size_t)n_utts + 1, &d_ooff));
    CHK(ws_grow(e, w.wave_off, (size_t)n_utts + 1, &d_woff));
    {   // the norm vectors stay on the device until the caller passes other values
        const size_t had = w.norm.cap;
        CHK(ws_grow(e, w.norm, (size_t)2 * d.D, &norm));
        std::vector<float> nv((size_t)2 * d.D);
        memcpy(nv.data(), norm_mean, d.D * sizeof(float));
        memcpy(nv.data() + d.D, norm_inv_std, d.D * sizeof(float));
        if (w.norm.cap != had || nv.size() != w.h_norm.size() ||
            memcmp(nv.data(), w.h_norm.data(), nv.size() * sizeof(float)) != 0) {
            HIPCHK(hipStreamSynchronize(st));  // no copy out of the old h_norm is in flight
            w.h_norm.swap(nv);
            HIPCHK(hipMemcpyAsync(norm, w.h_norm.data(), w.h_norm.size() * sizeof(float), hipMemcpyHostToDevice, st));
        }
    }
    const float *mean = norm, *inv = norm + d.D;
    HIPCHK(hipMemcpyAsync(dw, noisy + offsets[0], n_wave * sizeof(int16_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_foff, w.h_frame_off.data(), ((size_t)n_utts + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_ooff, w.h_out_off.data(), ((size_t)n_utts + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_woff, w.h_wave_off.data(), ((size_t)n_utts + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    if (w.lookup_table) {
        w.h_utt_of.resize(FT);
        for (int u = 0; u < n_utts; u++)
            std::fill(w.h_utt_of.begin() + w.h_frame_off[u], w.h_utt_of.begin() + w.h_frame_off[u + 1], u);
        CHK(ws_grow(e, w.utt_of, (size_t)FT, &d_utt));
        HIPCHK(hipMemcpyAsync(d_utt, w.h_utt_of.data(), (size_t)FT * sizeof(int), hipMemcpyHostToDevice, st));
    }
    CHK(launch_analysis_seg(p, dw, d_woff, d_foff, d_utt, n_utts, FT, dl, X, st));
    float *natz = nullptr;
    if (e->nat_frames) {  // every utterance's noise row, once per call, from the analysed rows of the whole batch
        CHK(ws_grow(e, w.nat, (size_t)n_utts * d.D, &natz));
        CHK(launch_nat_estimate(e, dl, d_foff, n_utts, d.D, mean, inv, natz));
    }
    // chunks over the packed frame index: a chunk's stream carries the context rows of every utterance it touches, so
    // an output frame sees the same input rows wherever the boundaries fall; bunches run across utterances
    for (int a = 0, u0 = 0; a < FT; a += cap) {
        const int n = std::min(cap, FT - a);
        const spec_rule::Span sp = spec_rule::chunk_span(w.h_frame_off.data(), &u0, a, n, fea_context);
        auto fill = [&](mlggd_engine::RawSet *r) -> int {
            hipLaunchKernelGGL(k_lps_stream_seg, dim3((unsigned)sp.rows), dim3(256), 0, st, dl, d_foff, d_utt, n_utts, d.D,
                               a, n, sp.u0, sp.u1, fea_context, mean, inv, r->feat.p, r->first.p);
            CHK(launch_check("k_lps_stream_seg"));
            if (!e->nat_frames) return MLGGD_OK;
            hipLaunchKernelGGL(k_nat_rows_seg, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const int *)d_foff,
                               (const int *)d_utt, n_utts, a, n, r->nat_row.p);
            return launch_check("k_nat_rows_seg");
        };
        CHK(decode_chunk(e, p, sp.rows, n, fea_context, fill, natz, mean, inv, gv_factors(e), X, a, blk, den, dl));
    }
    hipLaunchKernelGGL(k_ola_seg, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, blk, d_foff, d_ooff, n_utts,
                       p->d, p->win, of, oi, (long long)n_out);
    CHK(launch_check("k_ola_seg"));
    HIPCHK(hipMemcpyAsync(out, oi, n_out * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    if (out_f32) HIPCHK(hipMemcpyAsync(out_f32, of, n_out * sizeof(float), hipMemcpyDeviceToHost, st));
    if (lps_out) HIPCHK(hipMemcpyAsync(lps_out, den, (size_t)FT * d.D * sizeof(float), hipMemcpyDeviceToHost, st));
    if (clean) {  // the clean wave goes up once; 2 n_utts floats come back
        HIPCHK(hipMemcpyAsync(d_clean, clean + offsets[0], n_wave * sizeof(int16_t), hipMemcpyHostToDevice, st));
        if (score_frames)
            HIPCHK(hipMemcpyAsync(d_sf, score_frames, (size_t)n_utts * sizeof(int), hipMemcpyHostToDevice, st));
        CHK(launch_score(p, d_clean, d_woff, d_foff, d_utt, d_sf, n_utts, FT, den, X, Xc, fstat, scores, st));
        w.h_scores.resize((size_t)2 * n_utts);
        HIPCHK(hipMemcpyAsync(w.h_scores.data(), scores, (size_t)2 * n_utts * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    if (stoi) {  // the pass's own int16 output, still on the device, against the clean wave uploaded above
        HIPCHK(hipMemcpyAsync(sdev.utt, w.h_stoi_utt.data(), (size_t)n_utts * sizeof(StoiUtt), hipMemcpyHostToDevice, st));
        CHK(launch_stoi(splan, sfft, sjob, d_clean, oi, n_utts, sdev, st));
        w.h_stoi.resize((size_t)2 * n_utts);
        HIPCHK(hipMemcpyAsync(w.h_stoi.data(), sdev.res, (size_t)2 * n_utts * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (clean) {
        memcpy(segsnr, w.h_scores.data(), (size_t)n_utts * sizeof(float));
        memcpy(lsd, w.h_scores.data() + n_utts, (size_t)n_utts * sizeof(float));
    }
    if (stoi) stoi_results(w.h_stoi.data(), n_utts, stoi, segments);
    return MLGGD_OK;
}

int mlggd_enhance_waves(mlggd_handle e, int fs_khz, int fea_context, const float *norm_mean, const float *norm_inv_std,
                        int n_utts, const int16_t *noisy, const int64_t *offsets, int16_t *out, float *out_f32,
                        float *lps_out) {
    return enhance_waves_run(e, "mlggd_enhance_waves", fs_khz, fea_context, norm_mean, norm_inv_std, n_utts, noisy,
                             nullptr, offsets, nullptr, out, out_f32, lps_out, nullptr, nullptr);
}

int mlggd_enhance_waves_scored(mlggd_handle e, int fs_khz, int fea_context, const float *norm_mean,
                               const float *norm_inv_std, int n_utts, const int16_t *noisy, const int16_t *clean,
                               const int64_t *offsets, const int32_t *score_frames, int16_t *out, float *out_f32,
                               float *lps_out, float *segsnr, float *lsd) {
    if (e && n_utts > 0 && (!clean || !segsnr || !lsd)) return fail(MLGGD_ERR_ARG, "clean/segsnr/lsd is NULL");
    return enhance_waves_run(e, "mlggd_enhance_waves_scored", fs_khz, fea_context, norm_mean, norm_inv_std, n_utts,
                             noisy, clean, offsets, score_frames, out, out_f32, lps_out, segsnr, lsd);
}

int mlggd_score_waves(int device, int fs_khz, int n_utts, const int16_t *clean, const int16_t *noisy,
                      const int64_t *offsets, const float *lps, const int32_t *score_frames, float *segsnr, float *lsd) {
    SpecDims d;
    CHK(spec_dims(fs_khz, &d));
    if (n_utts < 0) return fail(MLGGD_ERR_ARG, "n_utts %d < 0", n_utts);
    if (n_utts == 0) return MLGGD_OK;
    if (!clean || !noisy || !offsets || !lps || !segsnr || !lsd)
        return fail(MLGGD_ERR_ARG, "clean/noisy/offsets/lps/segsnr/lsd is NULL");
    std::vector<int32_t> frame_off((size_t)n_utts + 1);
    std::vector<long long> wave_off((size_t)n_utts + 1);
    RULE(spec_rule::layout(d, n_utts, offsets, spec_rule::kShortFails, frame_off.data(), nullptr, wave_off.data(),
                           RULE_MSG));
    RULE(spec_rule::check_score_frames(n_utts, frame_off.data(), score_frames, RULE_MSG));
    const int FT = frame_off[n_utts];
    const size_t n_wave = (size_t)wave_off[n_utts];
    const SpecPlan *p;
    CHK(spec_plan_on(device, fs_khz, &p));
    DevBufs b;
    int16_t *dn = nullptr, *dc = nullptr;
    float *dl = nullptr, *fstat = nullptr, *scores = nullptr;
    float2 *X = nullptr, *Xc = nullptr;
    int *d_foff = nullptr, *d_sf = nullptr;
    long long *d_woff = nullptr;
    CHK(b.upload(&dn, noisy + offsets[0], n_wave));
    CHK(b.upload(&dc, clean + offsets[0], n_wave));
    CHK(b.upload(&dl, lps, (size_t)FT * d.D));
    CHK(b.alloc(&X, (size_t)FT * d.D));
    CHK(b.alloc(&Xc, (size_t)FT * d.D));
    CHK(b.alloc(&fstat, (size_t)3 * FT));
    CHK(b.alloc(&scores, (size_t)2 * n_utts));
    CHK(b.upload(&d_foff, frame_off.data(), (size_t)n_utts + 1));
    CHK(b.upload(&d_woff, wave_off.data(), (size_t)n_utts + 1));
    if (score_frames) CHK(b.upload(&d_sf, score_frames, (size_t)n_utts));
    CHK(launch_analysis_seg(p, dn, d_woff, d_foff, nullptr, n_utts, FT, nullptr, X, nullptr));
    CHK(launch_score(p, dc, d_woff, d_foff, nullptr, d_sf, n_utts, FT, dl, X, Xc, fstat, scores, nullptr));
    std::vector<float> h((size_t)2 * n_utts);
    HIPCHK(hipMemcpy(h.data(), scores, h.size() * sizeof(float), hipMemcpyDeviceToHost));
    memcpy(segsnr, h.data(), (size_t)n_utts * sizeof(float));
    memcpy(lsd, h.data() + n_utts, (size_t)n_utts * sizeof(float));
    return MLGGD_OK;
}

int mlggd_enhance_waves_scored_stoi(mlggd_handle e, int fs_khz, int fea_context, const float *norm_mean,
                                    const float *norm_inv_std, int n_utts, const int16_t *noisy, const int16_t *clean,
                                    const int64_t *offsets, const int32_t *score_frames, int16_t *out, float *out_f32,
                                    float *lps_out, float *segsnr, float *lsd, const int64_t *stoi_samples, float *stoi,
                                    int32_t *segments) {
    if (e && n_utts > 0 && (!clean || !segsnr || !lsd || !stoi))
        return fail(MLGGD_ERR_ARG, "clean/segsnr/lsd/stoi is NULL");
    return enhance_waves_run(e, "mlggd_enhance_waves_scored_stoi", fs_khz, fea_context, norm_mean, norm_inv_std, n_utts,
                             noisy, clean, offsets, score_frames, out, out_f32, lps_out, segsnr, lsd, stoi_samples, stoi,
                             segments);
}

int mlggd_stoi_layout(int fs_khz, int64_t n_samples, int64_t *len10, int64_t *frames, int64_t *min_segments) {
    int p, q, slot;
    if (!stoi_rule::rate(fs_khz, &p, &q, &slot)) return fail(MLGGD_ERR_ARG, "fs_khz %d: must be 8, 11 or 16", fs_khz);
    if (n_samples < 0 || n_samples > stoi_rule::kMaxSamples)
        return fail(MLGGD_ERR_ARG, "n_samples %lld is outside 0..%lld", (long long)n_samples,
                    (long long)stoi_rule::kMaxSamples);
    const int64_t l10 = stoi_rule::len10(n_samples, p, q), F = stoi_rule::frames(l10);
    if (len10) *len10 = l10;
    if (frames) *frames = F;
    if (min_segments) *min_segments = stoi_rule::segments(stoi_rule::compacted(F));
    return MLGGD_OK;
}

int mlggd_stoi_waves(int device, int fs_khz, int n_utts, const int16_t *clean, const int16_t *proc,
                     const int64_t *offsets, const int64_t *stoi_samples, float *stoi, int32_t *segments) {
    int p, q, slot;
    if (!stoi_rule::rate(fs_khz, &p, &q, &slot)) return fail(MLGGD_ERR_ARG, "fs_khz %d: must be 8, 11 or 16", fs_khz);
    if (n_utts < 0) return fail(MLGGD_ERR_ARG, "n_utts %d < 0", n_utts);
    if (n_utts == 0) return MLGGD_OK;
    if (!clean || !proc || !offsets || !stoi) return fail(MLGGD_ERR_ARG, "clean/proc/offsets/stoi is NULL");
    std::vector<long long> off((size_t)n_utts + 1), len((size_t)n_utts);
    RULE(spec_rule::layout(SpecDims(), n_utts, offsets, spec_rule::kUnframed, nullptr, nullptr, off.data(), RULE_MSG));
    for (int u = 0; u < n_utts; u++) len[u] = off[u + 1] - off[u];
    std::vector<StoiUtt> utt;
    StoiJob job;
    CHK(stoi_job(fs_khz, n_utts, off.data(), off.data(), len.data(), len.data(), stoi_samples, utt, &job));
    const size_t n_wave = (size_t)off[n_utts];
    HIPCHK(hipSetDevice(device));
    const StoiPlan *sp;
    const SpecPlan *fft;
    CHK(stoi_plan(device, &sp, &fft));
    DevBufs b;
    int16_t *dc = nullptr, *dp = nullptr;
    StoiDev sd = {};
    CHK(b.upload(&dc, clean + offsets[0], n_wave));
    CHK(b.upload(&dp, proc + offsets[0], n_wave));
    CHK(b.upload(&sd.utt, utt.data(), (size_t)n_utts));
    CHK(b.alloc(&sd.x, (size_t)2 * job.T10));
    CHK(b.alloc(&sd.f, (size_t)(1 + 2 * STOI_BANDS) * job.FT));
    CHK(b.alloc(&sd.i, (size_t)job.FT + n_utts));
    CHK(b.alloc(&sd.res, (size_t)2 * n_utts));
    CHK(launch_stoi(sp, fft, job, dc, dp, n_utts, sd, nullptr));
    std::vector<float> h((size_t)2 * n_utts);
    HIPCHK(hipMemcpy(h.data(), sd.res, h.size() * sizeof(float), hipMemcpyDeviceToHost));
    stoi_results(h.data(), n_utts, stoi, segments);
    return MLGGD_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ live groups (live.hip.h, live_rule.h)
// n_sessions audio sessions decoded block by block on one engine.  The sessions' state (live.hip.h) is the group's own
// device memory, in two copies; a push borrows from the engine only what mlggd_enhance_waves borrows for the time of
// one call -- the idle raw buffer set and chunk_out -- so training, decoding and set_weights between two pushes leave
// the sessions as they are.
struct mlggd_live {
    mlggd_engine *e = nullptr;
    int fs = 0, ctx = 0, half = 0, K = 0, NS = 0;
    SpecDims d;
    std::vector<long long> had;  // samples each session has received since it began
    int cur = 0;                 // the copy of the state that is current
    DevBuf<int16_t> tail[2];
    DevBuf<float> lps[2], blk[2], norm;
    DevBuf<float2> X[2];
    // the tables of one push, one block of pinned host memory and its device twin: win_off [NS + 1], out_off [NS + 1],
    // a_woff [NS] (long long), sess [NS], dk_off [NS + 1], dk_slot [NS], a_foff [NS + 1] (int)
    char *h_tab = nullptr;
    DevBuf<char> d_tab;
    size_t tab_bytes = 0;
    mlggd_engine::WsBuf in, win, lps_new, X_new, X_dec, blk_new, out_i, out_f;  // per push; they only grow
    std::vector<live_rule::Step> steps;
};

namespace {

struct LiveTables {
    long long *win_off, *out_off, *a_woff;
    LiveSess *sess;
    int *dk_off, *dk_slot, *a_foff;
};

size_t live_tables(char *base, int NS, LiveTables *t) {
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char *p = base + at;
        at += (bytes + 15) / 16 * 16;
        return p;
    };
    t->win_off = (long long *)take(((size_t)NS + 1) * sizeof(long long));
    t->out_off = (long long *)take(((size_t)NS + 1) * sizeof(long long));
    t->a_woff = (long long *)take((size_t)NS * sizeof(long long));
    t->sess = (LiveSess *)take((size_t)NS * sizeof(LiveSess));
    t->dk_off = (int *)take(((size_t)NS + 1) * sizeof(int));
    t->dk_slot = (int *)take((size_t)NS * sizeof(int));
    t->a_foff = (int *)take(((size_t)NS + 1) * sizeof(int));
    return at;
}

void live_free(mlggd_live *s) {
    if (s->h_tab) hipHostFree(s->h_tab);
    delete s;  // the device buffers free themselves; the caller has synchronised the engine's stream
}

int live_alloc(mlggd_live *s, const float *norm_mean, const float *norm_inv_std) {
    mlggd_engine *e = s->e;
    const SpecDims &d = s->d;
    const size_t NS = (size_t)s->NS;
    const size_t n_lps = std::max<size_t>(1, NS * (s->ctx - 1) * d.D), n_X = std::max<size_t>(1, NS * s->half * d.D);
    const size_t n_blk = NS * s->K * d.L, n_tail = NS * d.L;
    for (int c = 0; c < 2; c++) {
        HIPCHK(s->tail[c].grow(n_tail, n_tail, e->bufs, &e->stream, nullptr));
        HIPCHK(s->lps[c].grow(n_lps, n_lps, e->bufs, &e->stream, nullptr));
        HIPCHK(s->X[c].grow(n_X, n_X, e->bufs, &e->stream, nullptr));
        HIPCHK(s->blk[c].grow(n_blk, n_blk, e->bufs, &e->stream, nullptr));
    }
    HIPCHK(s->norm.grow((size_t)2 * d.D, (size_t)2 * d.D, e->bufs, nullptr, nullptr));
    HIPCHK(hipMemcpyAsync(s->norm.p, norm_mean, d.D * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(s->norm.p + d.D, norm_inv_std, d.D * sizeof(float), hipMemcpyHostToDevice, e->stream));
    LiveTables t;
    s->tab_bytes = live_tables(nullptr, s->NS, &t);
    HIPCHK(hipHostMalloc((void **)&s->h_tab, s->tab_bytes, hipHostMallocDefault));
    HIPCHK(s->d_tab.grow(s->tab_bytes, s->tab_bytes, e->bufs, nullptr, nullptr));
    memset(s->h_tab, 0, s->tab_bytes);
    HIPCHK(hipStreamSynchronize(e->stream));  // the norm vectors are the caller's
    return MLGGD_OK;
}

}  // namespace

extern "C" {

int mlggd_live_layout(int fs_khz, int fea_context, int n_sessions, const int64_t *had, const int64_t *add,
                      const uint8_t *end, int64_t *out_off) {
    RULE(live_rule::layout(fs_khz, fea_context, n_sessions, had, add, end, out_off, RULE_MSG));
    return MLGGD_OK;
}

int mlggd_live_open(mlggd_handle e, int fs_khz, int fea_context, const float *norm_mean, const float *norm_inv_std,
                    int n_sessions, mlggd_live_handle *out) {
    if (!e || !out) return fail(MLGGD_ERR_ARG, "NULL handle / out");
    *out = nullptr;
    if (e->nat_frames > 0)  // a session would have to hold its output back until nat_frames frames have arrived
        return fail(MLGGD_ERR_STATE, "mlggd_live_open: live decoding of an engine with nat_frames = %d is not built", e->nat_frames);
    if (e->mask_bins > 0)  // the post-filter reads the noisy LPS of the decoded frames: a second gathered ring
        return fail(MLGGD_ERR_STATE, "mlggd_live_open: live decoding of an engine with mask_bins = %d is not built", e->mask_bins);
    int L, S;
    RULE(live_rule::check_group(fs_khz, fea_context, n_sessions, &L, &S, RULE_MSG));
    SpecDims d;
    CHK(check_wave_engine(e, fs_khz, fea_context, true, &d));
    CHK(check_single_device(e, "mlggd_live_open", true));
    if (!norm_mean || !norm_inv_std) return fail(MLGGD_ERR_ARG, "norm_mean/norm_inv_std is NULL");
    if ((long long)n_sessions * (d.L + (long long)fea_context * d.D) > INT32_MAX / 2)
        return fail(MLGGD_ERR_ARG, "n_sessions %d is too large", n_sessions);
    const SpecPlan *p;
    CHK(spec_plan_on(e->device, fs_khz, &p));
    mlggd_live *s = new mlggd_live;
    s->e = e, s->fs = fs_khz, s->ctx = fea_context, s->half = (fea_context - 1) / 2, s->NS = n_sessions, s->d = d;
    s->K = (d.L + d.S - 1) / d.S - 1;
    s->had.assign((size_t)n_sessions, 0);
    s->steps.resize((size_t)n_sessions);
    const int rc = live_alloc(s, norm_mean, norm_inv_std);
    if (rc != MLGGD_OK) {
        live_free(s);
        return rc;
    }
    e->live_groups++;
    *out = s;
    return MLGGD_OK;
}

int mlggd_live_received(mlggd_live_handle s, int64_t *had) {
    if (!s || !had) return fail(MLGGD_ERR_ARG, "NULL handle / had");
    for (int u = 0; u < s->NS; u++) had[u] = s->had[u];
    return MLGGD_OK;
}

int mlggd_live_close(mlggd_live_handle s) {
    if (!s) return MLGGD_OK;
    mlggd_engine *e = s->e;
    hipSetDevice(e->device);
    hipStreamSynchronize(e->stream);
    e->live_groups--;
    live_free(s);
    return MLGGD_OK;
}

int mlggd_live_push(mlggd_live_handle s, const int16_t *samples, const int64_t *offsets, const uint8_t *end,
                    int16_t *out, float *out_f32, int64_t out_capacity, int64_t *out_off) {
    if (!s) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (!offsets || !out_off) return fail(MLGGD_ERR_ARG, "offsets/out_off is NULL");
    mlggd_engine *e = s->e;
    const SpecDims &d = s->d;
    const int NS = s->NS, ctx = s->ctx, half = s->half, K = s->K;
    // ---- the plan of the push, from the host's counters alone
    long long n_win = 0, n_emit = 0, NF = 0, ND = 0;
    for (int u = 0; u < NS; u++) {
        if (offsets[u + 1] < offsets[u])
            return fail(MLGGD_ERR_ARG, "offsets decrease at session %d (%lld after %lld)", u, (long long)offsets[u + 1],
                        (long long)offsets[u]);
        const long long add = (long long)offsets[u + 1] - (long long)offsets[u];
        if (add > live_rule::kMaxSamples - s->had[u])
            return fail(MLGGD_ERR_ARG, "session %d: %lld + %lld samples exceed the %lld one recording may have: end it", u,
                        s->had[u], add, (long long)live_rule::kMaxSamples);
        const live_rule::Step &st = s->steps[u] = live_rule::step(d.L, d.S, half, s->had[u], add, end && end[u]);
        n_win += st.p0 + add;
        n_emit += st.emit;
        NF += st.A1 - st.A0;
        ND += st.T1 - st.T0;
    }
    const long long n_in = (long long)offsets[NS] - (long long)offsets[0];
    if (n_in > 0 && !samples) return fail(MLGGD_ERR_ARG, "samples is NULL");
    if (n_emit > 0 && !out) return fail(MLGGD_ERR_ARG, "out is NULL");
    if (n_emit > out_capacity)
        return fail(MLGGD_ERR_ARG, "out_capacity %lld: the push emits %lld samples", (long long)out_capacity, n_emit);
    const int cap = chunk_cap(e);
    if (NF > INT32_MAX / 2 || ND > INT32_MAX / 2 ||
        std::min<long long>(cap, ND) + (long long)std::min(NS, cap) * (ctx - 1) > INT32_MAX / 2)
        return fail(MLGGD_ERR_ARG, "a push of %lld new frames over %d sessions is too large", std::max(NF, ND), NS);
    LiveTables h, dv;
    live_tables(s->h_tab, NS, &h);
    live_tables(s->d_tab.p, NS, &dv);
    int n_act = 0, n_dk = 0;
    h.win_off[0] = h.out_off[0] = 0;
    h.dk_off[0] = h.a_foff[0] = 0;
    out_off[0] = 0;
    for (int u = 0, nf_at = 0, dec_at = 0; u < NS; u++) {
        const live_rule::Step &st = s->steps[u];
        const long long add = (long long)offsets[u + 1] - (long long)offsets[u];
        const int nf = (int)(st.A1 - st.A0), nd = (int)(st.T1 - st.T0);
        LiveSess &q = h.sess[u];
        q.in_off = (long long)offsets[u] - (long long)offsets[0];
        q.p = (int)st.p0, q.a = (int)add, q.cut = nf * d.S;
        q.T0 = (int)st.T0, q.A0 = (int)st.A0, q.T1 = (int)st.T1, q.A1 = (int)st.A1;
        q.keep = (end && end[u]) ? 0 : 1;
        q.nf_off = nf_at, q.dec_off = dec_at;
        if (nf > 0) {  // the analysis batch: the sessions with new frames, their windows and frame offsets
            h.a_woff[n_act] = h.win_off[u];
            h.a_foff[++n_act] = nf_at + nf;
        }
        if (nd > 0) {
            h.dk_slot[n_dk] = u;
            h.dk_off[++n_dk] = dec_at + nd;
        }
        nf_at += nf, dec_at += nd;
        h.win_off[u + 1] = h.win_off[u] + st.p0 + add;
        h.out_off[u + 1] = h.out_off[u] + st.emit;
        out_off[u + 1] = h.out_off[u + 1];
    }
    // ---- the device
    const SpecPlan *p;
    CHK(spec_plan_on(e->device, s->fs, &p));
    hipStream_t st = e->stream;
    int16_t *d_in = nullptr, *d_win = nullptr, *oi = nullptr;
    float *lps_new = nullptr, *blk_new = nullptr, *of = nullptr;
    float2 *X_new = nullptr, *X_dec = nullptr;
    CHK(ws_grow(e, s->in, (size_t)n_in, &d_in));
    CHK(ws_grow(e, s->win, (size_t)n_win, &d_win));
    CHK(ws_grow(e, s->lps_new, (size_t)NF * d.D, &lps_new));
    CHK(ws_grow(e, s->X_new, (size_t)NF * d.D, &X_new));
    CHK(ws_grow(e, s->X_dec, (size_t)ND * d.D, &X_dec));
    CHK(ws_grow(e, s->blk_new, (size_t)ND * d.L, &blk_new));
    CHK(ws_grow(e, s->out_i, (size_t)n_emit, &oi));
    if (out_f32) CHK(ws_grow(e, s->out_f, (size_t)n_emit, &of));
    const int c0 = s->cur, c1 = s->cur ^ 1;
    const float *mean = s->norm.p, *inv = s->norm.p + d.D;
    if (n_in > 0)
        HIPCHK(hipMemcpyAsync(d_in, samples + offsets[0], (size_t)n_in * sizeof(int16_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->d_tab.p, s->h_tab, s->tab_bytes, hipMemcpyHostToDevice, st));
    if (n_win > 0) {
        hipLaunchKernelGGL(k_live_window, dim3((unsigned)((n_win + 255) / 256)), dim3(256), 0, st, d_in, s->tail[c0].p,
                           s->tail[c1].p, dv.sess, dv.win_off, NS, d.L, d_win, n_win);
        CHK(launch_check("k_live_window"));
    }
    if (NF > 0) CHK(launch_analysis_seg(p, d_win, dv.a_woff, dv.a_foff, nullptr, n_act, (int)NF, lps_new, X_new, st));
    if (ND > 0) {
        hipLaunchKernelGGL(k_live_gather_x, dim3((unsigned)ND), dim3(256), 0, st, s->X[c0].p, X_new, dv.sess, dv.dk_off,
                           dv.dk_slot, n_dk, d.D, half, X_dec);
        CHK(launch_check("k_live_gather_x"));
    }
    // chunks over the packed decoded frames, as in mlggd_enhance_waves
    for (int a = 0, k0 = 0; a < (int)ND; a += cap) {
        const int n = std::min(cap, (int)ND - a);
        const spec_rule::Span sp = spec_rule::chunk_span(h.dk_off, &k0, a, n, ctx);
        auto fill = [&](mlggd_engine::RawSet *r) {
            hipLaunchKernelGGL(k_live_stream, dim3((unsigned)sp.rows), dim3(256), 0, st, s->lps[c0].p, lps_new, dv.sess,
                               dv.dk_off, dv.dk_slot, n_dk, d.D, a, n, sp.u0, sp.u1, ctx, mean, inv, r->feat.p, r->first.p);
            return launch_check("k_live_stream");
        };
        CHK(decode_chunk(e, p, sp.rows, n, ctx, fill, nullptr, mean, inv, gv_factors(e), X_dec, a, blk_new, nullptr, nullptr));
    }
    if (n_emit > 0) {
        hipLaunchKernelGGL(k_live_ola, dim3((unsigned)((n_emit + 255) / 256)), dim3(256), 0, st, s->blk[c0].p, blk_new,
                           dv.sess, dv.out_off, NS, K, p->d, p->win, of, oi, n_emit);
        CHK(launch_check("k_live_ola"));
        HIPCHK(hipMemcpyAsync(out, oi, (size_t)n_emit * sizeof(int16_t), hipMemcpyDeviceToHost, st));
        if (out_f32) HIPCHK(hipMemcpyAsync(out_f32, of, (size_t)n_emit * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    hipLaunchKernelGGL(k_live_carry, dim3((unsigned)(NS * (ctx - 1 + half + K))), dim3(256), 0, st, dv.sess, ctx, K, d.D,
                       d.L, s->lps[c0].p, lps_new, s->lps[c1].p, s->X[c0].p, X_new, s->X[c1].p, s->blk[c0].p, blk_new, s->blk[c1].p);
    CHK(launch_check("k_live_carry"));
    HIPCHK(hipStreamSynchronize(st));
    s->cur = c1;
    for (int u = 0; u < NS; u++)
        s->had[u] = (end && end[u]) ? 0 : s->had[u] + ((long long)offsets[u + 1] - (long long)offsets[u]);
    return MLGGD_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ training data from waves (mix.hip.h, mix_rule.h)
// The mixer, the norm statistics and the wave-pair loader: int16 waves in, the raw set of the training loop out.
namespace {

// the tables of a batch over ALL its utterances; one shorter than a frame has no frames (that is no error here)
struct TrainLayout {
    std::vector<int32_t> frame_off;
    std::vector<long long> wave_off;
};
int train_layout(const SpecDims &d, int n_utts, const int64_t *offsets, TrainLayout *t) {
    t->frame_off.resize((size_t)n_utts + 1);
    t->wave_off.resize((size_t)n_utts + 1);
    RULE(spec_rule::layout(d, n_utts, offsets, spec_rule::kShortEmpty, t->frame_off.data(), nullptr, t->wave_off.data(),
                           RULE_MSG));
    return MLGGD_OK;
}

// the block table of a batch: utterance u in blocks of mix_rule::kBlock samples (one without samples has none)
void mix_blocks(int n_utts, const int64_t *offsets, const int64_t *lo, const int64_t *len, const int64_t *start,
                std::vector<mix_rule::Block> &out) {
    out.clear();
    for (int u = 0; u < n_utts; u++) {
        const long long n = (long long)offsets[u + 1] - (long long)offsets[u];
        for (long long i0 = 0; i0 < n; i0 += mix_rule::kBlock) {
            mix_rule::Block b;
            b.at = (long long)offsets[u] - (long long)offsets[0] + i0;
            b.lo = lo[u];
            b.len = len[u];
            b.phase = (long long)(((unsigned long long)start[u] + (unsigned long long)i0) % (unsigned long long)len[u]);
            b.n = (int)std::min<long long>(mix_rule::kBlock, n - i0);
            b.u = u;
            b.first = i0 == 0;
            b.pad = 0;
            out.push_back(b);
        }
    }
}

// the mixer's words per utterance in one device buffer: E [2 n] | r [n] | gain [n] | clipped [n]
struct MixUtt {
    unsigned long long *E;
    double *r, *gain;
    int *clipped;
    static size_t bytes(int n) { return (size_t)n * (16 + 8 + 8 + 4); }
    MixUtt(void *p, int n) {
        E = (unsigned long long *)p;
        r = (double *)(E + 2 * (size_t)n);
        gain = r + n;
        clipped = (int *)(gain + n);
    }
};

// both kernels over a block table on the device; the buffer of `m` is zeroed and r uploaded here
int launch_mix(const mix_rule::Block *d_blocks, int n_blocks, const int16_t *clean, const int16_t *noise, MixUtt m,
               int n_utts, const double *h_r, int16_t *noisy, hipStream_t st) {
    HIPCHK(hipMemsetAsync(m.E, 0, MixUtt::bytes(n_utts), st));
    HIPCHK(hipMemcpyAsync(m.r, h_r, (size_t)n_utts * sizeof(double), hipMemcpyHostToDevice, st));
    if (n_blocks == 0) return MLGGD_OK;
    hipLaunchKernelGGL(k_mix_energy, dim3((unsigned)n_blocks), dim3(MIX_THREADS), 0, st, d_blocks, clean, noise, m.E);
    CHK(launch_check("k_mix_energy"));
    hipLaunchKernelGGL(k_mix_apply, dim3((unsigned)n_blocks), dim3(MIX_THREADS), 0, st, d_blocks, clean, noise,
                       (const unsigned long long *)m.E, (const double *)m.r, noisy, m.gain, m.clipped);
    return launch_check("k_mix_apply");
}

void mix_ratios(int n_utts, const double *snr_db, std::vector<double> &r) {
    r.resize((size_t)n_utts);
    for (int u = 0; u < n_utts; u++) mix_rule::ratio(snr_db[u], &r[u]);  // checked before
}

// The checks of mlggd_load_waves / mlggd_cv_all_waves / mlggd_train_waves, all before any device call; *lay receives
// the layout over all utterances, *empty is set when there is nothing to load.
int wave_pair_check(mlggd_engine *e, const char *who, int fs_khz, int ctx, const float *mean, const float *inv, int n_utts,
                    const int64_t *offsets, int n_samples, const int32_t *first_frame, int targ_offset, SpecDims *d,
                    TrainLayout *lay, bool *empty) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    CHK(check_wave_engine(e, fs_khz, ctx, false, d));
    if (n_utts < 0) return fail(MLGGD_ERR_ARG, "n_utts %d < 0", n_utts);
    if (targ_offset < 0 || targ_offset >= ctx)
        return fail(MLGGD_ERR_ARG, "targ_offset %d not in [0, fea_context)", targ_offset);
    CHK(check_frames(e, n_samples));
    CHK(check_single_device(e, who, true));
    *empty = n_utts == 0 || n_samples == 0;
    if (*empty) return MLGGD_OK;
    if (!mean || !inv || !offsets || !first_frame) return fail(MLGGD_ERR_ARG, "norm/offsets/first_frame is NULL");
    CHK(train_layout(*d, n_utts, offsets, lay));
    RULE(spec_rule::check_windows(n_utts, lay->frame_off.data(), ctx, n_samples, first_frame, RULE_MSG));
    return MLGGD_OK;
}

// noisy / clean on the device (packed alike, index 0 = the batch's first sample) -> both analysed, normalised with the
// noisy statistics into the idle raw set, the sample table uploaded, the set made current.  Everything is enqueued on
// the engine's stream; the caller synchronises.
int wave_pair_load(mlggd_engine *e, const SpecDims &d, int fs_khz, int ctx, const float *mean, const float *inv,
                   const TrainLayout &lay, const int16_t *d_noisy, const int16_t *d_clean, int n_samples,
                   const int32_t *first_frame, int targ_offset) {
    mlggd_engine::TrainWs &t = e->tw;
    hipStream_t st = e->stream;
    const SpecPlan *p;
    CHK(spec_plan(e->device, fs_khz, &p));
    t.h_frame_off.resize(lay.frame_off.size());
    t.h_wave_off.resize(lay.frame_off.size());
    const int nc = spec_rule::compact_tables((int)lay.frame_off.size() - 1, lay.frame_off.data(), lay.wave_off.data(),
                                             t.h_frame_off.data(), t.h_wave_off.data());
    const int FT = lay.frame_off.back();
    float *lpsN = nullptr, *lpsC = nullptr, *norm = nullptr;
    int *d_foff = nullptr;
    long long *d_woff = nullptr;
    CHK(ws_grow(e, e->ww.lps, (size_t)FT * d.D, &lpsN));
    CHK(ws_grow(e, e->ww.lps_den, (size_t)FT * d.D, &lpsC));
    CHK(ws_grow(e, t.norm, (size_t)2 * d.D, &norm));
    CHK(ws_grow(e, t.frame_off, (size_t)nc + 1, &d_foff));
    CHK(ws_grow(e, t.wave_off, (size_t)nc + 1, &d_woff));
    mlggd_engine::RawSet *r;
    CHK(raw_set_acquire(e, FT, n_samples, ctx, nc, false, &r));
    t.h_norm.resize((size_t)2 * d.D);
    memcpy(t.h_norm.data(), mean, d.D * sizeof(float));
    memcpy(t.h_norm.data() + d.D, inv, d.D * sizeof(float));
    HIPCHK(hipMemcpyAsync(norm, t.h_norm.data(), t.h_norm.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_foff, t.h_frame_off.data(), ((size_t)nc + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_woff, t.h_wave_off.data(), ((size_t)nc + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(r->first.p, first_frame, (size_t)n_samples * sizeof(int), hipMemcpyHostToDevice, st));
    for (int k = 0; k < 2; k++)  // the spectrum itself is not wanted here: X = nullptr
        CHK(launch_analysis_seg(p, k ? d_clean : d_noisy, d_woff, d_foff, nullptr, nc, FT, k ? lpsC : lpsN, nullptr, st));
    if (e->mask_bins) {  // targ rows of 2 D floats: [normalised clean LPS | ratio mask]
        hipLaunchKernelGGL(k_lps_norm_pair_mask, dim3((unsigned)FT), dim3(256), 0, st, (const float *)lpsN,
                           (const float *)lpsC, d.D, (const float *)norm, (const float *)(norm + d.D), e->mask_scale,
                           r->feat.p, r->targ.p);
        CHK(launch_check("k_lps_norm_pair_mask"));
    } else {
        hipLaunchKernelGGL(k_lps_norm_pair, dim3((unsigned)FT), dim3(256), 0, st, (const float *)lpsN, (const float *)lpsC,
                           d.D, (const float *)norm, (const float *)(norm + d.D), r->feat.p, r->targ.p);
        CHK(launch_check("k_lps_norm_pair"));
    }
    if (e->nat_frames) {  // the noise rows from the normalised noisy rows, over the utterances that have frames
        CHK(launch_nat_estimate(e, r->feat.p, d_foff, nc, d.D, nullptr, nullptr, r->nat.p));
        t.h_nat_row.resize((size_t)n_samples);
        for (int s = 0; s < n_samples; s++)
            t.h_nat_row[s] = nat_rule::utt_of_frame(nc, t.h_frame_off.data(), first_frame[s]);
        HIPCHK(hipMemcpyAsync(r->nat_row.p, t.h_nat_row.data(), (size_t)n_samples * sizeof(int), hipMemcpyHostToDevice, st));
    }
    raw_set_commit(e, FT, n_samples, ctx, targ_offset);
    return MLGGD_OK;
}

// the packed waves of a batch into ww.wave (noisy, optional) / ww.clean
int upload_pair(mlggd_engine *e, const int16_t *noisy, const int16_t *clean, const int64_t *offsets, int n_utts,
                int16_t **d_noisy, int16_t **d_clean) {
    const size_t n_wave = (size_t)(offsets[n_utts] - offsets[0]);
    CHK(ws_grow(e, e->ww.wave, n_wave, d_noisy));
    CHK(ws_grow(e, e->ww.clean, n_wave, d_clean));
    if (noisy)
        HIPCHK(hipMemcpyAsync(*d_noisy, noisy + offsets[0], n_wave * sizeof(int16_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(*d_clean, clean + offsets[0], n_wave * sizeof(int16_t), hipMemcpyHostToDevice, e->stream));
    return MLGGD_OK;
}

}  // namespace

extern "C" {

int mlggd_wave_samples(int fs_khz, int fea_context, int n_utts, const int64_t *offsets, int32_t *first_frame,
                       int64_t *n_samples) {
    SpecDims d;
    CHK(spec_dims(fs_khz, &d));
    if (fea_context < 1) return fail(MLGGD_ERR_ARG, "fea_context %d < 1", fea_context);
    if (n_utts < 0) return fail(MLGGD_ERR_ARG, "n_utts %d < 0", n_utts);
    if (!n_samples) return fail(MLGGD_ERR_ARG, "n_samples is NULL");
    *n_samples = 0;
    if (n_utts == 0) return MLGGD_OK;
    if (!offsets) return fail(MLGGD_ERR_ARG, "offsets is NULL");
    TrainLayout lay;
    CHK(train_layout(d, n_utts, offsets, &lay));
    int64_t n = 0;
    for (int u = 0; u < n_utts; u++)
        for (int f = lay.frame_off[u]; f + fea_context <= lay.frame_off[u + 1]; f++, n++)
            if (first_frame) first_frame[n] = f;
    *n_samples = n;
    return MLGGD_OK;
}

int mlggd_mix_waves(int device, int n_utts, const int16_t *clean, const int64_t *offsets, const int16_t *noise,
                    int64_t n_noise, const int64_t *noise_lo, const int64_t *noise_len, const int64_t *noise_start,
                    const double *snr_db, int16_t *noisy, double *gain, int32_t *clipped) {
    if (n_utts < 0) return fail(MLGGD_ERR_ARG, "n_utts %d < 0", n_utts);
    if (n_utts == 0) return MLGGD_OK;
    if (!clean || !offsets || !noise || !noise_lo || !noise_len || !noise_start || !snr_db || !noisy)
        return fail(MLGGD_ERR_ARG, "clean/offsets/noise/noise_lo/noise_len/noise_start/snr_db/noisy is NULL");
    if (n_noise < 0) return fail(MLGGD_ERR_ARG, "n_noise %lld < 0", (long long)n_noise);
    RULE(mix_rule::check(n_utts, offsets, n_noise, noise_lo, noise_len, noise_start, snr_db, RULE_MSG));
    const size_t n_wave = (size_t)(offsets[n_utts] - offsets[0]);
    if (gain) std::fill(gain, gain + n_utts, 0.0);
    if (clipped) std::fill(clipped, clipped + n_utts, 0);
    if (n_wave == 0) return MLGGD_OK;
    std::vector<mix_rule::Block> blocks;
    std::vector<double> r;
    mix_blocks(n_utts, offsets, noise_lo, noise_len, noise_start, blocks);
    mix_ratios(n_utts, snr_db, r);
    HIPCHK(hipSetDevice(device));
    DevBufs b;
    int16_t *dc = nullptr, *dn = nullptr, *dz = nullptr;
    mix_rule::Block *db = nullptr;
    unsigned char *du = nullptr;
    CHK(b.upload(&dc, clean + offsets[0], n_wave));
    CHK(b.alloc(&dn, n_wave));
    CHK(b.upload(&dz, noise, (size_t)n_noise));
    CHK(b.upload(&db, blocks.data(), blocks.size()));
    CHK(b.alloc(&du, MixUtt::bytes(n_utts)));
    MixUtt m(du, n_utts);
    CHK(launch_mix(db, (int)blocks.size(), dc, dz, m, n_utts, r.data(), dn, nullptr));
    HIPCHK(hipMemcpy(noisy + offsets[0], dn, n_wave * sizeof(int16_t), hipMemcpyDeviceToHost));
    if (gain) HIPCHK(hipMemcpy(gain, m.gain, (size_t)n_utts * sizeof(double), hipMemcpyDeviceToHost));
    if (clipped) HIPCHK(hipMemcpy(clipped, m.clipped, (size_t)n_utts * sizeof(int), hipMemcpyDeviceToHost));
    return MLGGD_OK;
}

int mlggd_lps_stats(int device, int fs_khz, int n_utts, const int16_t *wave, const int64_t *offsets, double *sums,
                    int64_t *n_frames) {
    SpecDims d;
    CHK(spec_dims(fs_khz, &d));
    if (n_utts < 0) return fail(MLGGD_ERR_ARG, "n_utts %d < 0", n_utts);
    if (!sums || !n_frames) return fail(MLGGD_ERR_ARG, "sums/n_frames is NULL");
    if (n_utts > 0 && (!wave || !offsets)) return fail(MLGGD_ERR_ARG, "wave/offsets is NULL");
    TrainLayout lay;
    CHK(train_layout(d, n_utts, offsets, &lay));
    const int FT = lay.frame_off.back();
    std::fill(sums, sums + (size_t)2 * d.D, 0.0);
    *n_frames = FT;
    if (FT == 0) return MLGGD_OK;
    std::vector<int32_t> cf((size_t)n_utts + 1);
    std::vector<long long> cw((size_t)n_utts + 1);
    const int nc = spec_rule::compact_tables(n_utts, lay.frame_off.data(), lay.wave_off.data(), cf.data(), cw.data());
    const int chunks = (FT + CS_ROWS - 1) / CS_ROWS;
    const size_t n_wave = (size_t)lay.wave_off[n_utts];
    const SpecPlan *p;
    CHK(spec_plan_on(device, fs_khz, &p));
    DevBufs b;
    int16_t *dw = nullptr;
    float *dl = nullptr;
    double *part = nullptr, *ds = nullptr;
    int *d_foff = nullptr;
    long long *d_woff = nullptr;
    CHK(b.upload(&dw, wave + offsets[0], n_wave));
    CHK(b.alloc(&dl, (size_t)FT * d.D));
    CHK(b.alloc(&part, (size_t)chunks * 2 * d.D));
    CHK(b.alloc(&ds, (size_t)2 * d.D));
    CHK(b.upload(&d_foff, cf.data(), (size_t)nc + 1));
    CHK(b.upload(&d_woff, cw.data(), (size_t)nc + 1));
    CHK(launch_analysis_seg(p, dw, d_woff, d_foff, nullptr, nc, FT, dl, nullptr, nullptr));
    hipLaunchKernelGGL(k_lps_colstats, dim3((unsigned)((d.D + CS_BINS - 1) / CS_BINS), (unsigned)chunks), dim3(256), 0,
                       nullptr, (const float *)dl, FT, d.D, part);
    CHK(launch_check("k_lps_colstats"));
    hipLaunchKernelGGL(k_lps_colfold, dim3((unsigned)((2 * d.D + 255) / 256)), dim3(256), 0, nullptr,
                       (const double *)part, chunks, 2 * d.D, ds);
    CHK(launch_check("k_lps_colfold"));
    HIPCHK(hipMemcpy(sums, ds, (size_t)2 * d.D * sizeof(double), hipMemcpyDeviceToHost));
    return MLGGD_OK;
}

// the mask half of a mask engine's target rows from given un-normalised LPS rows: the device arithmetic of
// k_lps_norm_pair_mask, for users who build frame targets themselves
int mlggd_mask_targets(int device, int D, int64_t n_frames, const float *noisy_lps, const float *clean_lps, float scale,
                       float *out) {
    if (D < 1) return fail(MLGGD_ERR_ARG, "D %d < 1", D);
    if (n_frames < 0) return fail(MLGGD_ERR_ARG, "n_frames %lld < 0", (long long)n_frames);
    if (!(scale > 0.0f) || !std::isfinite(scale))
        return fail(MLGGD_ERR_ARG, "scale %g: must be positive and finite", (double)scale);
    if (n_frames == 0) return MLGGD_OK;
    if (!noisy_lps || !clean_lps || !out) return fail(MLGGD_ERR_ARG, "noisy_lps/clean_lps/out is NULL");
    const size_t n = (size_t)n_frames * (size_t)D;
    if ((n + 255) / 256 > (size_t)INT32_MAX) return fail(MLGGD_ERR_ARG, "n_frames %lld x %d bins is too large", (long long)n_frames, D);
    HIPCHK(hipSetDevice(device));
    DevBufs b;
    float *dn = nullptr, *dc = nullptr, *dt = nullptr;
    CHK(b.upload(&dn, noisy_lps, n));
    CHK(b.upload(&dc, clean_lps, n));
    CHK(b.alloc(&dt, n));
    hipLaunchKernelGGL(k_mask_targets, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, (const float *)dn,
                       (const float *)dc, n, scale, dt);
    CHK(launch_check("k_mask_targets"));
    HIPCHK(hipMemcpy(out, dt, n * sizeof(float), hipMemcpyDeviceToHost));
    return MLGGD_OK;
}

int mlggd_norm_from_stats(int D, int64_t n, const double *sums, float *mean, float *inv_std) {
    if (D < 1) return fail(MLGGD_ERR_ARG, "D %d < 1", D);
    if (n < 1) return fail(MLGGD_ERR_ARG, "n %lld < 1", (long long)n);
    if (!sums || !mean || !inv_std) return fail(MLGGD_ERR_ARG, "sums/mean/inv_std is NULL");
    for (int d = 0; d < D; d++) {
        const double m = sums[d] / (double)n;
        const double var = sums[(size_t)D + d] / (double)n - m * m;
        if (!(var > 0.0) || !std::isfinite(var))
            return fail(MLGGD_ERR_ARG, "bin %d: variance %g, no inverse standard deviation", d, var);
    }
    for (int d = 0; d < D; d++) {
        const double m = sums[d] / (double)n;
        const double var = sums[(size_t)D + d] / (double)n - m * m;
        mean[d] = (float)m;
        inv_std[d] = (float)(1.0 / sqrt(var));
    }
    return MLGGD_OK;
}

int mlggd_load_waves(mlggd_handle e, int fs_khz, int fea_context, const float *norm_mean, const float *norm_inv_std,
                     int n_utts, const int16_t *noisy, const int16_t *clean, const int64_t *offsets, int n_samples,
                     const int32_t *first_frame, int targ_offset) {
    SpecDims d;
    TrainLayout lay;
    bool empty = false;
    CHK(wave_pair_check(e, "mlggd_load_waves", fs_khz, fea_context, norm_mean, norm_inv_std, n_utts, offsets, n_samples,
                        first_frame, targ_offset, &d, &lay, &empty));
    if (empty) return MLGGD_OK;
    if (!noisy || !clean) return fail(MLGGD_ERR_ARG, "noisy/clean is NULL");
    HIPCHK(hipSetDevice(e->device));
    int16_t *dn = nullptr, *dc = nullptr;
    CHK(upload_pair(e, noisy, clean, offsets, n_utts, &dn, &dc));
    CHK(wave_pair_load(e, d, fs_khz, fea_context, norm_mean, norm_inv_std, lay, dn, dc, n_samples,
                       first_frame, targ_offset));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MLGGD_OK;
}

int mlggd_cv_all_waves(mlggd_handle e, int fs_khz, int fea_context, const float *norm_mean, const float *norm_inv_std,
                       int n_utts, const int16_t *noisy, const int16_t *clean, const int64_t *offsets, int n_samples,
                       const int32_t *first_frame, int targ_offset, float *sqerr, float *abserr, float *loglik) {
    SpecDims d;
    TrainLayout lay;
    bool empty = false;
    CHK(wave_pair_check(e, "mlggd_cv_all_waves", fs_khz, fea_context, norm_mean, norm_inv_std, n_utts, offsets,
                        n_samples, first_frame, targ_offset, &d, &lay, &empty));
    if (empty) {
        if (sqerr) *sqerr = 0.0f;
        if (abserr) *abserr = 0.0f;
        if (loglik) *loglik = 0.0f;
        return MLGGD_OK;
    }
    if (!noisy || !clean) return fail(MLGGD_ERR_ARG, "noisy/clean is NULL");
    HIPCHK(hipSetDevice(e->device));
    int16_t *dn = nullptr, *dc = nullptr;
    CHK(upload_pair(e, noisy, clean, offsets, n_utts, &dn, &dc));
    CHK(wave_pair_load(e, d, fs_khz, fea_context, norm_mean, norm_inv_std, lay, dn, dc, n_samples,
                       first_frame, targ_offset));
    std::vector<float> targ;
    if (!e->cv_device) {  // the host-order sums read the targets on the host: the normalised clean rows come back once
        targ.resize((size_t)lay.frame_off.back() * e->D);
        HIPCHK(hipMemcpyAsync(targ.data(), e->raw[e->raw_cur].targ.p, targ.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    const int rc = cv_indexed(e, n_samples, first_frame, targ_offset, targ.data(), sqerr, abserr, loglik);
    HIPCHK(hipEventRecord(e->raw[e->raw_cur].last_use, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return rc;
}

int mlggd_set_noise(mlggd_handle e, int64_t n_noise, const int16_t *noise) {
    if (!e) return fail(MLGGD_ERR_ARG, "NULL handle");
    if (n_noise < 0) return fail(MLGGD_ERR_ARG, "n_noise %lld < 0", (long long)n_noise);
    if (n_noise > 0 && !noise) return fail(MLGGD_ERR_ARG, "noise is NULL");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    mlggd_engine::TrainWs &t = e->tw;
    if (n_noise == 0 || !noise) {
        t.noise.release();
        t.n_noise = 0;
        return MLGGD_OK;
    }
    int16_t *dz = nullptr;
    t.n_noise = 0;
    CHK(ws_grow(e, t.noise, (size_t)n_noise, &dz));
    HIPCHK(hipMemcpyAsync(dz, noise, (size_t)n_noise * sizeof(int16_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    t.n_noise = n_noise;
    return MLGGD_OK;
}

int mlggd_train_waves(mlggd_handle e, int fs_khz, int fea_context, const float *norm_mean, const float *norm_inv_std,
                      int n_utts, const int16_t *clean, const int64_t *offsets, const int64_t *noise_lo,
                      const int64_t *noise_len, const int64_t *noise_start, const double *snr_db, int n_samples,
                      const int32_t *first_frame, int targ_offset, int16_t *noisy_out, double *gain, int32_t *clipped,
                      int *bunches_trained) {
    if (bunches_trained) *bunches_trained = 0;
    SpecDims d;
    TrainLayout lay;
    bool empty = false;
    CHK(wave_pair_check(e, "mlggd_train_waves", fs_khz, fea_context, norm_mean, norm_inv_std, n_utts, offsets, n_samples,
                        first_frame, targ_offset, &d, &lay, &empty));
    mlggd_engine::TrainWs &t = e->tw;
    if (!t.noise.p || t.n_noise == 0)
        return fail(MLGGD_ERR_STATE, "mlggd_train_waves: the engine has no noise bank (mlggd_set_noise)");
    if (empty) return MLGGD_OK;
    if (!clean || !noise_lo || !noise_len || !noise_start || !snr_db)
        return fail(MLGGD_ERR_ARG, "clean/noise_lo/noise_len/noise_start/snr_db is NULL");
    RULE(mix_rule::check(n_utts, offsets, t.n_noise, noise_lo, noise_len, noise_start, snr_db, RULE_MSG));
    mix_blocks(n_utts, offsets, noise_lo, noise_len, noise_start, t.h_blocks);
    mix_ratios(n_utts, snr_db, t.h_r);
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const size_t n_wave = (size_t)(offsets[n_utts] - offsets[0]);
    int16_t *dn = nullptr, *dc = nullptr;
    mix_rule::Block *db = nullptr;
    unsigned char *du = nullptr;
    CHK(upload_pair(e, nullptr, clean, offsets, n_utts, &dn, &dc));
    CHK(ws_grow(e, t.blocks, t.h_blocks.size(), &db));
    CHK(ws_grow(e, t.utt, MixUtt::bytes(n_utts), &du));
    MixUtt m(du, n_utts);
    HIPCHK(hipMemcpyAsync(db, t.h_blocks.data(), t.h_blocks.size() * sizeof(mix_rule::Block), hipMemcpyHostToDevice, st));
    CHK(launch_mix(db, (int)t.h_blocks.size(), dc, (const int16_t *)t.noise.p, m, n_utts, t.h_r.data(), dn, st));
    if (noisy_out)
        HIPCHK(hipMemcpyAsync(noisy_out + offsets[0], dn, n_wave * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    if (gain) HIPCHK(hipMemcpyAsync(gain, m.gain, (size_t)n_utts * sizeof(double), hipMemcpyDeviceToHost, st));
    if (clipped) HIPCHK(hipMemcpyAsync(clipped, m.clipped, (size_t)n_utts * sizeof(int), hipMemcpyDeviceToHost, st));
    CHK(wave_pair_load(e, d, fs_khz, fea_context, norm_mean, norm_inv_std, lay, dn, dc, n_samples,
                       first_frame, targ_offset));
    CHK(mlggd_train_resident(e, 0, n_samples, bunches_trained));
    return mlggd_sync(e);
}

}  // extern "C"

// the mask engine's kernels (declared in spectral.hip.h and mix.hip.h)
#include "mask.hip.h"
#include "rbm.hip.h"
