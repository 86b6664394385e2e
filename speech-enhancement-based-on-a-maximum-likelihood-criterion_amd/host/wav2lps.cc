// wav2lps.cc -- drop-in for the original project's Wav2LPS_be (Feature_prepare/SourceCode_Wav2LogSpec_be): 16-bit
// wave in, log-power spectra out as a big-endian HTK file (nframes, 160000, 4 (N/2+1), 9), computed on the GPU by
// mlggd_wave_to_lps.  The command lines of LPS_extract.m and decode.m work unchanged.
//
//   wav2lps [-q] [-F RAW|WAV] [-fs 8|11|16] [-swap] [-noh] [-gpu N] infile outfile
//
// RAW (the default): headerless samples in the machine's byte order (-swap: the other one), rate from -fs (16).
// WAV: RIFF PCM16 mono, rate from the file.  NIST / HTK input and -win > 0 are refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tool_io.h"

[[noreturn]] void die(const std::string &m) {
    fprintf(stderr, "wav2lps: %s\n", m.c_str());
    exit(1);
}

int main(int argc, char **argv) {
    std::string kind = "RAW", in, out;
    int fs = 16, gpu = 0;
    bool quiet = false, swap = false, noh = false;
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
        else if (arg == "-noh") noh = true;
        else if (arg == "-gpu") gpu = atoi(value().c_str());
        else if (arg == "-win") {
            if (atoi(value().c_str()) != 0) die("-win > 0 (stacked output frames) is not supported");
        } else if (arg == "-noc0" || arg == "-nologE") {
        } else if (arg.size() > 1 && arg[0] == '-') fprintf(stderr, "WARNING:  Un-recognized flag '%s' !\n", arg.c_str());
        else if (in.empty()) in = arg;
        else if (out.empty()) out = arg;
        else die("too many input arguments");
    }
    if (in.empty() || out.empty())
        die("usage: wav2lps [-q] [-F RAW|WAV] [-fs 8|11|16] [-swap] [-noh] [-gpu N] infile outfile");
    std::vector<int16_t> wave;
    if (kind == "RAW") {
        wave = tool_io::read_raw16(in, swap);
    } else if (kind == "WAV") {
        int rate = 0;
        wave = tool_io::read_wav(in, &rate);
        fs = tool_io::rate_khz(rate);
        if (!fs) die(in + ": sample rate " + std::to_string(rate) + " Hz is not 8000, 11000 or 16000");
    } else if (kind == "NIST" || kind == "HTK") {
        die("input format " + kind + " is not supported: convert to RAW or WAV");
    } else {
        die("invalid input file format '" + kind + "'");
    }
    if (fs != 8 && fs != 11 && fs != 16) die("invalid sampling frequency " + std::to_string(fs) + " kHz");
    int F = 0;
    if (mlggd_wave_to_lps(gpu, fs, (int)wave.size(), wave.data(), &F, nullptr) != MLGGD_OK)
        die(std::string("mlggd_wave_to_lps: ") + mlggd_last_error());
    int L, S, N;
    tool_io::spectral_params(fs, &L, &S, &N);
    std::vector<float> lps((size_t)F * (N / 2 + 1));
    if (F > 0 && mlggd_wave_to_lps(gpu, fs, (int)wave.size(), wave.data(), &F, lps.data()) != MLGGD_OK)
        die(std::string("mlggd_wave_to_lps: ") + mlggd_last_error());
    tool_io::write_htk(out, lps.data(), F, N / 2 + 1, !noh);
    if (!quiet) fprintf(stderr, "Processed: %d Frames.\n", F);
    return 0;
}
