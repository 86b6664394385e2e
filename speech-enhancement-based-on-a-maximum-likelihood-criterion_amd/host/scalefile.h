// scalefile.h -- the state of the learned scale (mlggd_set_scale_mode, csrc/scale_rule.h) as a text file, so that the
// trainer can carry it from one epoch's process to the next (MLGGD_SCALE_FILE=PATH, read in train_options.cc): a .wts file has
// no place for alpha.  Also behind mlggd_read_scale_state / mlggd_write_scale_state.  Not in the reference: the 28-key
// command line and the log file do not change.  No dependency on mlggd.h.
//
//   # learned GGD scale ...
//   # D 257
//   # lrate 0.05
//   # momentum 0.5
//   # vmax 1
//   # steps 1234
//   # d alpha velocity
//   0 0.81234567 -0.00012345678
//   ...
// Every number is printed with %.9g, which names every float uniquely: a round trip keeps every bit.  The reader skips
// '#' lines and takes the rows 0..D-1 in order, three fields each.  alpha must be finite and not negative (0: the bin
// seeds from its first minibatch), the velocity finite.  Every refusal is *err = "PATH line N: what is wrong" -- a wrong
// count is named at the file's last line, an unreadable file at line 1 -- and leaves the output unspecified.
#pragma once
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace mlggd_host {

struct ScaleFileHeader {
    float lrate, momentum, vmax;
    long long steps;
};

inline bool scalefile_bad(const std::string &path, long line, const std::string &what, std::string *err) {
    *err = path + " line " + std::to_string(line) + ": " + what;
    return false;
}

inline bool write_scale_state(const std::string &path, int D, const float *alpha, const float *velocity,
                              const ScaleFileHeader &h, std::string *err) {
    FILE *fp = fopen(path.c_str(), "w");
    if (!fp) return scalefile_bad(path, 1, "cannot write the file", err);
    fprintf(fp, "# learned GGD scale: per output bin, alpha moved by SGD with momentum on ln alpha, and its velocity\n");
    fprintf(fp, "# D %d\n# lrate %.9g\n# momentum %.9g\n# vmax %.9g\n# steps %lld\n# d alpha velocity\n", D, (double)h.lrate,
            (double)h.momentum, (double)h.vmax, h.steps);
    for (int d = 0; d < D; d++) fprintf(fp, "%d %.9g %.9g\n", d, (double)alpha[d], velocity ? (double)velocity[d] : 0.0);
    if (fclose(fp) != 0) return scalefile_bad(path, (long)D + 7, "cannot write the file", err);
    return true;
}

// alpha[D] and velocity[D] (velocity may be nullptr) from `path`; steps (may be nullptr): the header's "# steps N", 0
// without one
inline bool parse_scale_state(const std::string &path, int D, float *alpha, float *velocity, std::string *err,
                              long long *steps = nullptr) {
    auto bad = [&](long line, const std::string &what) { return scalefile_bad(path, line, what, err); };
    FILE *fp = fopen(path.c_str(), "r");
    if (!fp) return bad(1, "cannot read the file");
    std::vector<std::string> lines;
    {
        std::string cur;
        int c;
        while ((c = fgetc(fp)) != EOF) {
            if (c == '\n') {
                lines.push_back(cur);
                cur.clear();
            } else {
                cur.push_back((char)c);
            }
        }
        if (!cur.empty()) lines.push_back(cur);
        fclose(fp);
    }
    const long last = lines.empty() ? 1 : (long)lines.size();
    const std::string sD = std::to_string(D);
    int row = 0;
    if (steps) *steps = 0;
    for (size_t li = 0; li < lines.size(); li++) {
        const std::string &l = lines[li];
        std::vector<std::string> f;
        for (size_t i = 0; i < l.size();) {
            while (i < l.size() && isspace((unsigned char)l[i])) i++;
            size_t j = i;
            while (j < l.size() && !isspace((unsigned char)l[j])) j++;
            if (j > i) f.push_back(l.substr(i, j - i));
            i = j;
        }
        if (f.empty()) continue;
        if (f[0][0] == '#') {
            if (steps && f.size() == 3 && f[0] == "#" && f[1] == "steps") *steps = atoll(f[2].c_str());
            continue;
        }
        const long ln = (long)li + 1;
        if (row == D) return bad(ln, "more than the " + sD + " rows of the output layer");
        if (f.size() < 3) return bad(ln, "a row has the fields d alpha velocity, this one has " + std::to_string(f.size()));
        double v[3];
        for (int k = 0; k < 3; k++) {
            char *end = nullptr;
            v[k] = strtod(f[k].c_str(), &end);
            if (end == f[k].c_str() || *end != 0) return bad(ln, "field " + std::to_string(k + 1) + " '" + f[k] + "' is not a number");
        }
        if (v[0] != (double)row) return bad(ln, "row " + f[0] + " where row " + std::to_string(row) + " belongs");
        const float a = (float)v[1], vel = (float)v[2];
        if (!std::isfinite(a) || a < 0.0f) return bad(ln, "alpha " + f[1] + " of bin " + std::to_string(row) + " is negative or not finite");
        if (!std::isfinite(vel)) return bad(ln, "velocity " + f[2] + " of bin " + std::to_string(row) + " is not finite");
        alpha[row] = a;
        if (velocity) velocity[row] = vel;
        row++;
    }
    if (row != D) return bad(last, std::to_string(row) + " rows, the output layer has " + sD);
    return true;
}

}  // namespace mlggd_host
