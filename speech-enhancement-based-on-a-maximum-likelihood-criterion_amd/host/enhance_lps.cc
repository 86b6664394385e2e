// enhance_lps.cc -- batch inference: the forward pass of the reference's
// MATLAB decoder (Test_code/decode.m:10-63) on the MI355X engine, without MATLAB:
//   noisy LPS (HTK big-endian, Test_code/readHTK_new.m) -> z-normalise with the training norm
//   file (decode.m:31-33) -> edge-replicated context of fea_context frames
//   (Test_code/frame_expand.m:5-27) -> sigmoid MLP from the trainer's .wts (decode.m:11-18,
//   39-57) -> de-normalise (decode.m:59-61) -> HTK file with sampPeriod 160000, sampSize 4*D,
//   paramKind 9 (decode.m:62, Test_code/writeHTK_new.m:36-51).
// The edge-replicated windows become contiguous slices of a stream padded with (ctx-1)/2 copies
// of the first / last frame, so the forward runs through mlggd_forward_frames.
//
//   enhance_lps wts=mlp.50.wts norm_file=train_noisy.norm in=noisy.lps out=enhanced.htk
//               [fea_context=7] [gpu_used=0] [bunchsize=512] [scp=list of "in out" lines] [activation=sigmoid|relu] [nat=T]
//               [gv=FILE [gv_mode=bin|shared]]
// activation: the hidden units the net was trained with (BPtrain_Sigmoid / BPtrain_ReLU); the .wts file does not say.
// nat=T: the net was trained noise-aware (csrc/nat_rule.h): every input row ends in the mean of the file's first T
// normalised frames, layersizes[0] = (fea_context + 1) x the feature dimension; the .wts file does not say that either.
// gv=FILE: global variance equalisation (csrc/gv_rule.h): output bin j of the net is multiplied by the factor FILE
// holds for it (a plain list or the file an epoch with MLGGD_GVFILE=FILE wrote; gv_mode=shared: the file's one factor
// for all bins) before it is de-normalised.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "tool_io.h"

[[noreturn]] void die(const std::string &m) {
    fprintf(stderr, "enhance_lps: %s\n", m.c_str());
    exit(1);
}

using tool_io::Htk;
using tool_io::read_htk;
using tool_io::write_htk;

int main(int argc, char **argv) {
    std::string wts, norm_file, in, out, scp, gv, gv_mode = "bin";
    int ctx = 7, gpu = 0, bunch = 512, act = MLGGD_ACT_SIGMOID, nat = 0;
    for (int a = 1; a < argc; a++) {
        const std::string arg(argv[a]);
        const size_t eq = arg.find('=');
        if (eq == std::string::npos) die("Arg: " + arg + "  Format Error");
        const std::string k = arg.substr(0, eq), v = arg.substr(eq + 1);
        if (k == "wts") wts = v;
        else if (k == "norm_file") norm_file = v;
        else if (k == "in") in = v;
        else if (k == "out") out = v;
        else if (k == "scp") scp = v;
        else if (k == "fea_context") ctx = atoi(v.c_str());
        else if (k == "gpu_used") gpu = atoi(v.c_str());
        else if (k == "bunchsize") bunch = atoi(v.c_str());
        else if (k == "activation") act = tool_io::parse_activation(v);
        else if (k == "nat") nat = tool_io::parse_nat(v);
        else if (k == "gv") gv = v;
        else if (k == "gv_mode") gv_mode = v;
    }
    if (wts.empty() || norm_file.empty() || (scp.empty() && (in.empty() || out.empty())))
        die("usage: enhance_lps wts=F norm_file=F (in=F out=F | scp=LIST) [fea_context=7] [gpu_used=0] [bunchsize=512] [activation=sigmoid|relu] [nat=T] [gv=FILE [gv_mode=bin|shared]]");
    if (ctx < 1 || ctx % 2 == 0) die("fea_context must be odd");

    // ---- model: the trainer's .wts container (Interface.cc:484-516)
    const tool_io::Model model = tool_io::read_wts(wts);
    const std::vector<int> &ls = model.ls;
    const int L = (int)ls.size(), D = ls[L - 1];
    const int parts = ctx + (nat > 0 ? 1 : 0);
    if (ls[0] % parts) die(nat > 0 ? "layersizes[0] is not a multiple of fea_context + 1 (nat=)" : "layersizes[0] is not a multiple of fea_context");
    const int dim = ls[0] / parts;

    // ---- norm file (Interface.cc:373-399 layout: "vec N", N means, "vec N", N inverse std-devs)
    std::vector<float> mean, inv;
    tool_io::read_norm(norm_file, dim, mean, inv);
    if (D % dim) die("output dimension is not a multiple of the feature dimension");

    const std::vector<float> eta = tool_io::read_gv_arg(gv, gv_mode, D);  // a bad file ends the run before the engine exists
    mlggd_handle h = tool_io::create_engine(model, gpu, bunch, 0, act, nat);

    std::vector<std::pair<std::string, std::string>> jobs;
    if (!scp.empty()) {
        std::ifstream f(scp);
        if (!f) die("cannot open " + scp);
        std::string a, b;
        while (f >> a >> b) jobs.emplace_back(a, b);
    } else {
        jobs.emplace_back(in, out);
    }
    const int half = (ctx - 1) / 2;
    for (const auto &job : jobs) {
        const Htk x = read_htk(job.first);
        if (x.samp_size != dim * 4) die(job.first + ": feature dimension does not match the model");
        const int n = x.nframes, np = n + 2 * half;
        std::vector<float> stream((size_t)np * dim);
        for (int t = 0; t < np; t++) {  // frame_expand.m: clamp to the first / last frame
            int src = t - half;
            src = src < 0 ? 0 : (src >= n ? n - 1 : src);
            for (int j = 0; j < dim; j++) stream[(size_t)t * dim + j] = (x.data[(size_t)src * dim + j] - mean[j]) * inv[j];
        }
        std::vector<int32_t> first(n);
        for (int t = 0; t < n; t++) first[t] = t;
        std::vector<float> y((size_t)n * D);
        if (nat > 0) {  // the noise row from the file's own normalised rows (stream rows half .. half + n)
            const int32_t foff[2] = {0, n};
            std::vector<float> z(dim);
            std::vector<int32_t> zrow(n, 0);
            if (mlggd_nat_estimate(dim, 1, foff, stream.data() + (size_t)half * dim, nat, z.data()) != MLGGD_OK ||
                mlggd_forward_frames_nat(h, np, ctx, stream.data(), n, first.data(), 1, z.data(), zrow.data(), y.data()) !=
                    MLGGD_OK)
                die(std::string("mlggd_forward_frames_nat: ") + mlggd_last_error());
        } else if (mlggd_forward_frames(h, np, ctx, stream.data(), n, first.data(), y.data()) != MLGGD_OK)
            die(std::string("mlggd_forward_frames: ") + mlggd_last_error());
        for (int t = 0; t < n; t++)
            for (int j = 0; j < D; j++) {  // decode.m:59-61; with gv= the factor first (csrc/gv_rule.h), one rounding each
                const float v = y[(size_t)t * D + j];
                const float s = eta.empty() ? v : v * eta[j];
                const float q = s / inv[j % dim];
                y[(size_t)t * D + j] = q + mean[j % dim];
            }
        write_htk(job.second, y.data(), n, D);
        printf("%s -> %s (%d frames)\n", job.first.c_str(), job.second.c_str(), n);
    }
    mlggd_destroy(h);
    return 0;
}
