// mix_wav.cc -- noisy training waves from clean speech and noise at an SNR, mixed on the GPU by mlggd_mix_waves (the
// rule is csrc/mix_rule.h), and the norm file of what was written.  The original project ships no mixer.
//
//   mix_wav scp=LIST [norm_out=FILE] [fs=16] [gpu_used=0] [batch_s=300]
//
// Every line of LIST is `clean.wav noise.wav snr_db start out.wav`: RIFF PCM16 mono files at fs kHz; the noise file
// is the utterance's noise segment, read from sample `start` on and wrapping at its end; snr_db may be `inf`.  Lines
// are mixed a batch (up to batch_s seconds of clean speech) per pass over the device; a noise file that several lines
// of a batch name goes up once.  One line per utterance is printed: the output file, the gain, the clipped samples.
// norm_out=: mlggd_lps_stats of the written waves is added up over the batches and the norm file of the trainer and
// the decoders is written -- `vec D`, the means, `vec D`, the inverse standard deviations (population variance), %g.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "tool_io.h"

[[noreturn]] void die(const std::string &m) {
    fprintf(stderr, "mix_wav: %s\n", m.c_str());
    exit(1);
}

static const char *kUsage = "usage: mix_wav scp=LIST [norm_out=FILE] [fs=16] [gpu_used=0] [batch_s=300]";

struct Line {
    std::string clean, noise, out;
    double snr_db;
    long long start;
};

int main(int argc, char **argv) {
    std::string scp, norm_out;
    int fs = 16, gpu = 0;
    double batch_s = 300.0;
    for (int a = 1; a < argc; a++) {
        const std::string arg(argv[a]);
        const size_t eq = arg.find('=');
        const std::string key = arg.substr(0, eq), val = eq == std::string::npos ? "" : arg.substr(eq + 1);
        if (key == "scp") scp = val;
        else if (key == "norm_out") norm_out = val;
        else if (key == "fs") fs = atoi(val.c_str());
        else if (key == "gpu_used") gpu = atoi(val.c_str());
        else if (key == "batch_s") batch_s = atof(val.c_str());
        else die("unknown argument " + arg + "\n" + kUsage);
    }
    if (scp.empty()) die(kUsage);
    if (fs != 8 && fs != 11 && fs != 16) die("invalid sampling frequency " + std::to_string(fs) + " kHz");
    if (!(batch_s > 0)) die("batch_s must be positive");
    std::vector<Line> lines;
    {
        std::ifstream f(scp);
        if (!f) die("cannot open " + scp);
        std::string text;
        for (int no = 1; std::getline(f, text); no++) {
            std::istringstream ss(text);
            Line l;
            std::string snr, start;
            if (!(ss >> l.clean)) continue;  // an empty line
            if (!(ss >> l.noise >> snr >> start >> l.out))
                die(scp + " line " + std::to_string(no) + ": expected `clean.wav noise.wav snr_db start out.wav`");
            char *end = nullptr;
            l.snr_db = strtod(snr.c_str(), &end);
            if (end == snr.c_str() || *end) die(scp + " line " + std::to_string(no) + ": snr_db '" + snr + "' is no number");
            l.start = strtoll(start.c_str(), &end, 10);
            if (end == start.c_str() || *end) die(scp + " line " + std::to_string(no) + ": start '" + start + "' is no integer");
            lines.push_back(l);
        }
    }
    int L, S, N;
    tool_io::spectral_params(fs, &L, &S, &N);
    const int D = N / 2 + 1;
    const int hz = fs == 16 ? 16000 : fs == 11 ? 11000 : 8000;
    auto read = [&](const std::string &path) {
        int rate = 0;
        std::vector<int16_t> w = tool_io::read_wav(path, &rate);
        if (rate != hz) die(path + ": sample rate " + std::to_string(rate) + " Hz, expected " + std::to_string(hz));
        return w;
    };
    std::vector<double> sums((size_t)2 * D, 0.0), part((size_t)2 * D);
    int64_t n_frames = 0;
    for (size_t at = 0; at < lines.size();) {
        // one batch: lines [at, to), their clean waves packed, their noise files packed once each
        std::vector<int16_t> clean, noise;
        std::vector<int64_t> off(1, 0), lo, len, start;
        std::vector<double> snr;
        std::map<std::string, std::pair<int64_t, int64_t>> bank;
        size_t to = at;
        while (to < lines.size() && (to == at || (double)clean.size() < batch_s * hz)) {
            const Line &l = lines[to++];
            const std::vector<int16_t> c = read(l.clean);
            clean.insert(clean.end(), c.begin(), c.end());
            off.push_back((int64_t)clean.size());
            auto it = bank.find(l.noise);
            if (it == bank.end()) {
                const std::vector<int16_t> z = read(l.noise);
                it = bank.emplace(l.noise, std::make_pair((int64_t)noise.size(), (int64_t)z.size())).first;
                noise.insert(noise.end(), z.begin(), z.end());
            }
            lo.push_back(it->second.first);
            len.push_back(it->second.second);
            start.push_back(l.start);
            snr.push_back(l.snr_db);
        }
        const int n = (int)(to - at);
        std::vector<int16_t> noisy(clean.size() ? clean.size() : 1);
        std::vector<double> gain(n);
        std::vector<int32_t> clipped(n);
        if (clean.empty()) clean.push_back(0);
        if (noise.empty()) noise.push_back(0);
        if (mlggd_mix_waves(gpu, n, clean.data(), off.data(), noise.data(), (int64_t)(noise.size()), lo.data(), len.data(),
                            start.data(), snr.data(), noisy.data(), gain.data(), clipped.data()) != MLGGD_OK)
            die(std::string("mlggd_mix_waves (lines from ") + lines[at].out + "): " + mlggd_last_error());
        for (int u = 0; u < n; u++) {
            tool_io::write_wav(lines[at + u].out, noisy.data() + off[u], (size_t)(off[u + 1] - off[u]), hz);
            printf("%s gain %.17g clipped %d\n", lines[at + u].out.c_str(), gain[u], (int)clipped[u]);
        }
        if (!norm_out.empty()) {
            int64_t nf = 0;
            if (mlggd_lps_stats(gpu, fs, n, noisy.data(), off.data(), part.data(), &nf) != MLGGD_OK)
                die(std::string("mlggd_lps_stats: ") + mlggd_last_error());
            for (size_t i = 0; i < sums.size(); i++) sums[i] += part[i];
            n_frames += nf;
        }
        at = to;
    }
    if (!norm_out.empty()) {
        std::vector<float> mean(D), inv(D);
        if (mlggd_norm_from_stats(D, n_frames, sums.data(), mean.data(), inv.data()) != MLGGD_OK)
            die(std::string("mlggd_norm_from_stats: ") + mlggd_last_error());
        FILE *fp = fopen(norm_out.c_str(), "wt");
        if (!fp) die("cannot open " + norm_out + " for writing");
        fprintf(fp, "vec %d\n", D);
        for (int d = 0; d < D; d++) fprintf(fp, "%g\n", (double)mean[d]);
        fprintf(fp, "vec %d\n", D);
        for (int d = 0; d < D; d++) fprintf(fp, "%g\n", (double)inv[d]);
        fclose(fp);
        fprintf(stderr, "mix_wav: norm file %s from %lld frames\n", norm_out.c_str(), (long long)n_frames);
    }
    return 0;
}
