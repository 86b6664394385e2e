// lps2wav.cc -- drop-in for the original project's LPS2Wav_be (Test_code/SourceCode_LogSpec2Wav_be, OLA_KIND 1):
// LPS rows (big-endian HTK) + the noisy wave's phase -> 16-bit wave by overlap-add, on the GPU (mlggd_lps_to_wave),
// and the quality report against the clean wave (segmental SNR, log-spectral distortion) in the original's format.
//
//   lps2wav clean noisy feat.htk info.txt out [-F RAW|WAV] [-fs 8|11|16] [-swap] [-q] [-gpu N] [score=host|device]
//
// score=host (the default): the report in double on the host; score=device: in fp32 on the GPU (mlggd_score_waves).
// The argument order of LogSpec2Wav.c:233-290.  RAW (the default) writes headerless samples, WAV a RIFF file.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tool_io.h"

[[noreturn]] void die(const std::string &m) {
    fprintf(stderr, "lps2wav: %s\n", m.c_str());
    exit(1);
}

int main(int argc, char **argv) {
    std::string kind = "RAW", score = "host";
    const char *usage =
        "usage: lps2wav clean noisy feat.htk info.txt out [-F RAW|WAV] [-fs 8|11|16] [-swap] [-gpu N] [score=host|device]";
    std::vector<std::string> files;
    int fs = 16, gpu = 0;
    bool swap = false, quiet = false;
    for (int a = 1; a < argc; a++) {
        const std::string arg(argv[a]);
        auto value = [&]() -> std::string {
            if (a + 1 >= argc) die("option " + arg + " needs a value");
            return argv[++a];
        };
        if (arg == "-q") quiet = true;
        else if (arg == "-F") kind = value();
        else if (arg == "-fs") fs = atoi(value().c_str());
        else if (arg == "-swap") swap = true;
        else if (arg == "-gpu") gpu = atoi(value().c_str());
        else if (arg.compare(0, 6, "score=") == 0) score = arg.substr(6);
        else if (arg.size() > 1 && arg[0] == '-') fprintf(stderr, "WARNING:  Un-recognized flag '%s' !\n", arg.c_str());
        else files.push_back(arg);
    }
    if (files.size() != 5) die(usage);
    if (score != "host" && score != "device") die("score=" + score + ": must be host or device\n" + usage);
    std::vector<int16_t> clean, noisy;
    if (kind == "RAW") {
        clean = tool_io::read_raw16(files[0], swap);
        noisy = tool_io::read_raw16(files[1], swap);
    } else if (kind == "WAV") {
        int r0 = 0, r1 = 0;
        clean = tool_io::read_wav(files[0], &r0);
        noisy = tool_io::read_wav(files[1], &r1);
        if (r0 != r1) die("clean and noisy sample rates differ");
        fs = tool_io::rate_khz(r0);
        if (!fs) die(files[0] + ": sample rate " + std::to_string(r0) + " Hz is not 8000, 11000 or 16000");
    } else if (kind == "NIST" || kind == "HTK") {
        die("input format " + kind + " is not supported: convert to RAW or WAV");
    } else {
        die("invalid input file format '" + kind + "'");
    }
    if (fs != 8 && fs != 11 && fs != 16) die("invalid sampling frequency " + std::to_string(fs) + " kHz");
    int L, S, N;
    tool_io::spectral_params(fs, &L, &S, &N);
    const int D = N / 2 + 1;
    const tool_io::Htk feat = tool_io::read_htk(files[2]);
    if (feat.samp_size != 4 * D) die(files[2] + ": feature dimension is not " + std::to_string(D));
    // frames while both waves have samples (LogSpec2Wav.c:577-580)
    auto frames = [&](size_t n) { return n < (size_t)L ? 0 : (int)((n - (L - S)) / S); };
    const int F = std::min(frames(clean.size()), frames(noisy.size()));
    if (F == 0) die("the waves are shorter than one frame");
    if (feat.nframes < F) die(files[2] + ": " + std::to_string(feat.nframes) + " frames, the waves have " + std::to_string(F));
    const size_t n_out = (size_t)F * S + L - S;
    std::vector<int16_t> out(n_out);
    if (mlggd_lps_to_wave(gpu, fs, (int)n_out, noisy.data(), F, feat.data.data(), out.data(), nullptr) != MLGGD_OK)
        die(std::string("mlggd_lps_to_wave: ") + mlggd_last_error());
    double segsnr = 0.0, lsd = 0.0;
    if (score == "device") {  // one utterance of F frames: both waves hold its n_out samples
        const int64_t off[2] = {0, (int64_t)n_out};
        float s = 0.0f, l = 0.0f;
        if (mlggd_score_waves(gpu, fs, 1, clean.data(), noisy.data(), off, feat.data.data(), nullptr, &s, &l) != MLGGD_OK)
            die(std::string("mlggd_score_waves: ") + mlggd_last_error());
        segsnr = s, lsd = l;
    } else {
        tool_io::quality(fs, clean, noisy, feat.data.data(), F, &segsnr, &lsd);
    }
    tool_io::write_info(files[3], segsnr, lsd);
    if (kind == "WAV")
        tool_io::write_wav(files[4], out.data(), n_out, fs == 11 ? 11000 : fs * 1000);
    else
        tool_io::write_raw16(files[4], out.data(), n_out);
    if (!quiet) fprintf(stderr, "Processed: %d Frames.\n", F);
    return 0;
}
