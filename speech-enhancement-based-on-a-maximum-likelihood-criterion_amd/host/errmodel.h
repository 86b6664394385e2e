// errmodel.h -- the trainer's opt-in error-model report (MLGGD_ERRMODEL=FILE, bptrain_main.cc): the shape grid of
// MLGGD_ERRMODEL_BETAS and the text file written from the CV set's error statistics (mlggd_error_stats over every CV
// chunk, added, then mlggd_ggd_fit), and the reader of that file for MLGGD_SHAPEFACTORS=FILE (parse_shapefactors,
// also behind mlggd_read_shapefactors).  Not in the reference: the 28-key command line and the log file do not change.
#pragma once
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mlggd.h"

namespace mlggd_host {

// "lo:step:hi" (nullptr / empty: 0.5:0.1:2.5) -> beta_i = (float)(lo + i * step), the sum evaluated in double, while
// <= hi + step / 2.  At most MLGGD_MAX_BETAS values; every error names the variable.
inline std::vector<float> beta_grid(const char *spec) {
    double lo = 0.5, step = 0.1, hi = 2.5;
    if (spec && *spec) {
        char tail = 0;
        if (sscanf(spec, "%lf:%lf:%lf%c", &lo, &step, &hi, &tail) != 3)
            throw std::runtime_error(std::string("MLGGD_ERRMODEL_BETAS=") + spec + ": expected lo:step:hi");
        if (!(lo > 0) || !(step > 0) || !(hi >= lo) || !std::isfinite(lo) || !std::isfinite(step) || !std::isfinite(hi))
            throw std::runtime_error(std::string("MLGGD_ERRMODEL_BETAS=") + spec + ": needs 0 < lo <= hi and step > 0");
    }
    std::vector<float> betas;
    for (int i = 0; lo + i * step <= hi + step / 2; i++) {
        if ((int)betas.size() == MLGGD_MAX_BETAS)
            throw std::runtime_error(std::string("MLGGD_ERRMODEL_BETAS=") + (spec && *spec ? spec : "0.5:0.1:2.5") +
                                     ": more than " + std::to_string(MLGGD_MAX_BETAS) + " shapes");
        betas.push_back((float)(lo + i * step));
    }
    return betas;
}

// The fit of `sums` ([4 + K][D], added over the CV chunks, n samples) as text: '#' header lines with n, D, the grid,
// shared_beta and loglik_per_frame for every grid beta, then one row per bin
//   d mean var kurt best_beta alpha_at_best alpha_at_shared
// in %.9g (a bin without a fit: best_beta nan, both alpha 0).  Returns the shared beta (NaN: no bin has a fit).
inline double write_error_model(const std::string &path, int D, int64_t n, const std::vector<float> &betas,
                                const std::vector<double> &sums) {
    const int K = (int)betas.size();
    std::vector<double> mean(D), var(D), kurt(D), alpha((size_t)K * D), shared(K);
    std::vector<int32_t> best(D);
    int32_t bs = -1;
    if (mlggd_ggd_fit(D, n, K, betas.data(), sums.data(), mean.data(), var.data(), kurt.data(), alpha.data(), nullptr,
                      best.data(), shared.data(), &bs) != MLGGD_OK)
        throw std::runtime_error(std::string("mlggd_ggd_fit failed: ") + mlggd_last_error());
    FILE *fp = fopen(path.c_str(), "w");
    if (!fp) throw std::runtime_error("MLGGD_ERRMODEL: cannot write " + path);
    const double shared_beta = bs >= 0 ? (double)betas[bs] : std::nan("");
    fprintf(fp, "# GGD error model of the CV set: beta/(2 alpha Gamma(1/beta)) exp(-(|e|/alpha)^beta), e = out - targ\n");
    fprintf(fp, "# n %lld\n# D %d\n# betas", (long long)n, D);
    for (int k = 0; k < K; k++) fprintf(fp, " %.9g", (double)betas[k]);
    fprintf(fp, "\n# shared_beta %.9g\n# loglik_per_frame", shared_beta);
    for (int k = 0; k < K; k++) fprintf(fp, " %.9g", shared[k] / (double)n);
    fprintf(fp, "\n# d mean var kurt best_beta alpha_at_best alpha_at_shared\n");
    for (int d = 0; d < D; d++)
        fprintf(fp, "%d %.9g %.9g %.9g %.9g %.9g %.9g\n", d, mean[d], var[d], kurt[d],
                best[d] >= 0 ? (double)betas[best[d]] : std::nan(""), best[d] >= 0 ? alpha[(size_t)best[d] * D + d] : 0.0,
                bs >= 0 ? alpha[(size_t)bs * D + d] : 0.0);
    if (fclose(fp) != 0) throw std::runtime_error("MLGGD_ERRMODEL: cannot write " + path);
    return shared_beta;
}

// The way back (MLGGD_SHAPEFACTORS=FILE, mlggd_read_shapefactors): one shape per output bin from either
//   - a plain list: exactly D numbers separated by white space, any number per line, or
//   - the file write_error_model writes: '#' lines are skipped (a finite '# shared_beta' is remembered), the data rows
//     must be rows 0..D-1 in order and field 5 of row d, best_beta, is bin d's shape.  A 'nan' there marks a bin
//     without a fit; it takes the file's shared beta, or `fallback` when the file has none.
// A file is taken for an error model when a '#' line comes before its first number, or when its first data line has
// five or more fields and starts with the row number 0 (no list can start with 0: every shape is positive).
// Returns false with *err = "PATH line N: what is wrong" on a wrong count, a row out of order, a field that is no
// number and a shape that is not positive and finite; betas is then unspecified.
inline bool parse_shapefactors(const std::string &path, int D, float fallback, float *betas, std::string *err) {
    auto bad = [&](long line, const std::string &what) {
        *err = path + " line " + std::to_string(line) + ": " + what;
        return false;
    };
    FILE *fp = fopen(path.c_str(), "r");
    if (!fp) {
        *err = "cannot read " + path;
        return false;
    }
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
    auto fields = [](const std::string &l) {
        std::vector<std::string> f;
        size_t i = 0;
        while (i < l.size()) {
            while (i < l.size() && isspace((unsigned char)l[i])) i++;
            size_t j = i;
            while (j < l.size() && !isspace((unsigned char)l[j])) j++;
            if (j > i) f.push_back(l.substr(i, j - i));
            i = j;
        }
        return f;
    };
    auto number = [](const std::string &t, double *v) {
        char *end = nullptr;
        *v = strtod(t.c_str(), &end);
        return end != t.c_str() && *end == 0;
    };
    auto shape_ok = [](double v) { return (float)v > 0.0f && std::isfinite((float)v); };
    // which of the two formats
    bool model = false;
    for (const std::string &l : lines) {
        const std::vector<std::string> f = fields(l);
        if (f.empty()) continue;
        if (f[0][0] == '#') model = true;
        else if (f.size() >= 5 && f[0] == "0") model = true;
        break;
    }
    const long last = (long)lines.size() > 0 ? (long)lines.size() : 1;
    if (!model) {
        int n = 0;
        for (size_t li = 0; li < lines.size(); li++) {
            const std::vector<std::string> f = fields(lines[li]);
            if (!f.empty() && f[0][0] == '#') continue;
            for (const std::string &t : f) {
                double v;
                if (!number(t, &v)) return bad((long)li + 1, "'" + t + "' is not a number");
                if (n == D) return bad((long)li + 1, "more than the " + std::to_string(D) + " shapes of the output layer");
                if (!shape_ok(v)) return bad((long)li + 1, "shape " + t + " of bin " + std::to_string(n) + " is not positive and finite");
                betas[n++] = (float)v;
            }
        }
        if (n != D) return bad(last, std::to_string(n) + " shapes, the output layer has " + std::to_string(D));
        return true;
    }
    double shared = std::nan("");
    std::vector<int> unfit;
    int row = 0;
    for (size_t li = 0; li < lines.size(); li++) {
        const std::vector<std::string> f = fields(lines[li]);
        if (f.empty()) continue;
        if (f[0][0] == '#') {
            const size_t k = f[0] == "#" ? 1 : 0;  // "# shared_beta X" or "#shared_beta X"
            if (f.size() > k + 1 && (f[k] == "shared_beta" || f[k] == "#shared_beta")) {
                double v;
                if (!number(f[k + 1], &v)) return bad((long)li + 1, "shared_beta '" + f[k + 1] + "' is not a number");
                if (std::isfinite(v)) {
                    if (!shape_ok(v)) return bad((long)li + 1, "shared_beta " + f[k + 1] + " is not positive and finite");
                    shared = v;
                }
            }
            continue;
        }
        if (row == D) return bad((long)li + 1, "more than the " + std::to_string(D) + " rows of the output layer");
        if (f.size() < 5) return bad((long)li + 1, "a row has the fields d mean var kurt best_beta ..., this one has " + std::to_string(f.size()));
        double v[5];
        for (int k = 0; k < 5; k++)
            if (!number(f[k], &v[k])) return bad((long)li + 1, "field " + std::to_string(k + 1) + " '" + f[k] + "' is not a number");
        if (v[0] != (double)row) return bad((long)li + 1, "row " + f[0] + " where row " + std::to_string(row) + " belongs");
        if (std::isnan(v[4])) {
            unfit.push_back(row);
        } else {
            if (!shape_ok(v[4])) return bad((long)li + 1, "best_beta " + f[4] + " of bin " + std::to_string(row) + " is not positive and finite");
            betas[row] = (float)v[4];
        }
        row++;
    }
    if (row != D) return bad(last, std::to_string(row) + " rows, the output layer has " + std::to_string(D));
    for (int d : unfit) betas[d] = std::isnan(shared) ? fallback : (float)shared;
    return true;
}

}  // namespace mlggd_host
