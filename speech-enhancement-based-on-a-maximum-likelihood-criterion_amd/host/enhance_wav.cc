// enhance_wav.cc -- the whole of the original project's decoder (Test_code/decode.m) in one process: noisy RIFF
// WAV -> LPS -> z-normalise with the training norm file -> edge-replicated context of fea_context frames -> sigmoid
// MLP from the trainer's .wts -> de-normalise -> overlap-add resynthesis with the noisy phase -> enhanced RIFF WAV,
// all on the GPU by mlggd_enhance_wave.  With clean= and info=, the quality report of LPS2Wav_be against the clean
// wave (its LPS is the de-normalised network output, formed again from the public pieces on the same engine).
//
//   enhance_wav wts=mlp.wts norm_file=train_noisy.norm (in=noisy.wav out=enhanced.wav | scp=LIST)
//               [fea_context=7] [gpu_used=0] [bunchsize=512] [clean=clean.wav info=info.txt]
//
// scp lists "in out" lines, like enhance_lps.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "tool_io.h"

[[noreturn]] void die(const std::string &m) {
    fprintf(stderr, "enhance_wav: %s\n", m.c_str());
    exit(1);
}

int main(int argc, char **argv) {
    std::string wts, norm_file, in, out, scp, clean, info;
    int ctx = 7, gpu = 0, bunch = 512;
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
        else if (k == "clean") clean = v;
        else if (k == "info") info = v;
        else if (k == "fea_context") ctx = atoi(v.c_str());
        else if (k == "gpu_used") gpu = atoi(v.c_str());
        else if (k == "bunchsize") bunch = atoi(v.c_str());
        else die("unknown argument " + k);
    }
    if (wts.empty() || norm_file.empty() || (scp.empty() && (in.empty() || out.empty())))
        die("usage: enhance_wav wts=F norm_file=F (in=F out=F | scp=LIST) [fea_context=7] [gpu_used=0] [bunchsize=512] "
            "[clean=F info=F]");
    if (ctx < 1 || ctx % 2 == 0) die("fea_context must be odd");
    if (clean.empty() != info.empty()) die("clean= and info= go together");
    if (!clean.empty() && !scp.empty()) die("clean= / info= need a single in= / out= pair");

    const tool_io::Model model = tool_io::read_wts(wts);
    const int D = model.ls.back();
    if (model.ls[0] != ctx * D) die("layersizes[0] is not fea_context x the output dimension");
    std::vector<float> mean, inv;
    tool_io::read_norm(norm_file, D, mean, inv);
    mlggd_handle h = tool_io::create_engine(model, gpu, bunch);

    std::vector<std::pair<std::string, std::string>> jobs;
    if (!scp.empty()) {
        std::ifstream f(scp);
        if (!f) die("cannot open " + scp);
        std::string a, b;
        while (f >> a >> b) jobs.emplace_back(a, b);
    } else {
        jobs.emplace_back(in, out);
    }
    for (const auto &job : jobs) {
        int rate = 0;
        const std::vector<int16_t> noisy = tool_io::read_wav(job.first, &rate);
        const int fs = tool_io::rate_khz(rate);
        if (!fs) die(job.first + ": sample rate " + std::to_string(rate) + " Hz is not 8000, 11000 or 16000");
        int L, S, N;
        tool_io::spectral_params(fs, &L, &S, &N);
        if (noisy.size() < (size_t)L) die(job.first + ": shorter than one frame");
        const int F = (int)((noisy.size() - (L - S)) / S);
        std::vector<int16_t> enh((size_t)F * S + L - S);
        int n_out = 0;
        if (mlggd_enhance_wave(h, fs, ctx, mean.data(), inv.data(), (int)noisy.size(), noisy.data(), enh.data(), nullptr,
                               &n_out) != MLGGD_OK)
            die(std::string("mlggd_enhance_wave: ") + mlggd_last_error());
        tool_io::write_wav(job.second, enh.data(), (size_t)n_out, rate);
        printf("%s -> %s (%d frames)\n", job.first.c_str(), job.second.c_str(), F);
        if (!clean.empty()) {
            // the enhanced LPS rows: the same chain through the public pieces (decode.m:31-61)
            std::vector<float> lps((size_t)F * D);
            int Fq = 0;
            if (mlggd_wave_to_lps(gpu, fs, (int)noisy.size(), noisy.data(), &Fq, lps.data()) != MLGGD_OK)
                die(std::string("mlggd_wave_to_lps: ") + mlggd_last_error());
            const int half = (ctx - 1) / 2, np = F + 2 * half;
            std::vector<float> stream((size_t)np * D);
            for (int t = 0; t < np; t++) {
                const int src = std::min(std::max(t - half, 0), F - 1);
                for (int j = 0; j < D; j++) stream[(size_t)t * D + j] = (lps[(size_t)src * D + j] - mean[j]) * inv[j];
            }
            std::vector<int32_t> first(F);
            for (int t = 0; t < F; t++) first[t] = t;
            std::vector<float> y((size_t)F * D);
            if (mlggd_forward_frames(h, np, ctx, stream.data(), F, first.data(), y.data()) != MLGGD_OK)
                die(std::string("mlggd_forward_frames: ") + mlggd_last_error());
            for (size_t i = 0; i < y.size(); i++) y[i] = y[i] / inv[i % D] + mean[i % D];
            int cr = 0;
            const std::vector<int16_t> cw = tool_io::read_wav(clean, &cr);
            if (cr != rate) die(clean + ": sample rate differs from " + job.first);
            const int Fc = cw.size() < (size_t)L ? 0 : (int)((cw.size() - (L - S)) / S);
            const int Fm = std::min(F, Fc);
            if (Fm == 0) die(clean + ": shorter than one frame");
            double segsnr = 0.0, lsd = 0.0;
            tool_io::quality(fs, cw, noisy, y.data(), Fm, &segsnr, &lsd);
            tool_io::write_info(info, segsnr, lsd);
        }
    }
    mlggd_destroy(h);
    return 0;
}
