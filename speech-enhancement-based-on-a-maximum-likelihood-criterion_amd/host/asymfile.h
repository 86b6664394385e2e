// asymfile.h -- the trainer's opt-in fit of the asymmetric GGD error model (MLGGD_ASYMMODEL=FILE, bptrain_main.cc): the
// text file written from the CV set's signed error statistics (mlggd_error_stats_signed over every CV chunk, added,
// then mlggd_asym_fit over the grid of MLGGD_ERRMODEL_BETAS), and the reader of that file for MLGGD_ASYMMETRY=FILE
// (parse_asymmetry, also behind mlggd_read_asymmetry).  Not in the reference: the 28-key command line and the log file
// do not change.
//
// The row layout is chosen so that the SAME file reads as a shape file through parse_shapefactors (errmodel.h) as it
// is: '#' header lines with a '# shared_beta' among them, rows 0..D-1 in order, five or more numeric fields, field 5
// best_beta.  best_kappa is the next field:
//   d p_plus p_minus alpha_at_best best_beta best_kappa alpha_at_shared kappa_at_shared
// p_plus / p_minus are P+ / n and P- / n at the bin's best shape.  One fit then feeds
// MLGGD_SHAPEFACTORS=fit.txt MLGGD_ASYMMETRY=fit.txt in the next epoch.
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

// The fit of `sums` ([2 K][D], added over the CV chunks, n samples) as text, every number in %.9g.  A bin without a
// fit: best_beta and best_kappa nan, the other fields 0.  Returns the shared beta (NaN: no bin has a fit).
inline double write_asym_model(const std::string &path, int D, int64_t n, const std::vector<float> &betas,
                               const std::vector<double> &sums) {
    const int K = (int)betas.size();
    std::vector<double> kappa((size_t)K * D), alpha((size_t)K * D), shared(K);
    std::vector<int32_t> best(D);
    int32_t bs = -1;
    if (mlggd_asym_fit(D, n, K, betas.data(), sums.data(), kappa.data(), alpha.data(), nullptr, best.data(), shared.data(),
                       &bs) != MLGGD_OK)
        throw std::runtime_error(std::string("mlggd_asym_fit failed: ") + mlggd_last_error());
    FILE *fp = fopen(path.c_str(), "w");
    if (!fp) throw std::runtime_error("MLGGD_ASYMMODEL: cannot write " + path);
    const double shared_beta = bs >= 0 ? (double)betas[bs] : std::nan("");
    fprintf(fp, "# asymmetric GGD error model of the CV set: beta/(alpha (kappa + 1/kappa) Gamma(1/beta)) exp(-(s(e)/alpha)^beta),\n");
    fprintf(fp, "# e = out - targ, s(e) = kappa e for e > 0, -e / kappa for e < 0\n");
    fprintf(fp, "# n %lld\n# D %d\n# betas", (long long)n, D);
    for (int k = 0; k < K; k++) fprintf(fp, " %.9g", (double)betas[k]);
    fprintf(fp, "\n# shared_beta %.9g\n# loglik_per_frame", shared_beta);
    for (int k = 0; k < K; k++) fprintf(fp, " %.9g", shared[k] / (double)n);
    fprintf(fp, "\n# d p_plus p_minus alpha_at_best best_beta best_kappa alpha_at_shared kappa_at_shared\n");
    const double nan = std::nan("");
    for (int d = 0; d < D; d++) {
        const int b = best[d];
        const bool sh = bs >= 0 && !std::isnan(kappa[(size_t)bs * D + d]);  // this bin has a fit at the shared shape
        fprintf(fp, "%d %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", d, b >= 0 ? sums[(size_t)b * D + d] / (double)n : 0.0,
                b >= 0 ? sums[(size_t)(K + b) * D + d] / (double)n : 0.0, b >= 0 ? alpha[(size_t)b * D + d] : 0.0,
                b >= 0 ? (double)betas[b] : nan, b >= 0 ? kappa[(size_t)b * D + d] : nan,
                sh ? alpha[(size_t)bs * D + d] : 0.0, sh ? kappa[(size_t)bs * D + d] : nan);
    }
    if (fclose(fp) != 0) throw std::runtime_error("MLGGD_ASYMMODEL: cannot write " + path);
    return shared_beta;
}

// The way back (MLGGD_ASYMMETRY=FILE, mlggd_read_asymmetry): one skew per output bin from either
//   - a plain list: exactly D numbers separated by white space, any number per line, or
//   - the file write_asym_model writes: '#' lines are skipped, the data rows must be rows 0..D-1 in order and field 6
//     of row d, best_kappa, is bin d's skew.  A 'nan' there marks a bin without a fit; it takes `fallback`.
// A file is taken for a model file when a '#' line comes before its first number, or when its first data line has six
// or more fields and starts with the row number 0 (no list can start with 0: every skew is positive).
// Returns false with *err = "PATH line N: what is wrong" on a wrong count, a row out of order, a field that is no
// number and a skew that is not positive and finite; kappas is then unspecified.
inline bool parse_asymmetry(const std::string &path, int D, float fallback, float *kappas, std::string *err) {
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
    auto skew_ok = [](double v) { return (float)v > 0.0f && std::isfinite((float)v); };
    bool model = false;
    for (const std::string &l : lines) {
        const std::vector<std::string> f = fields(l);
        if (f.empty()) continue;
        if (f[0][0] == '#') model = true;
        else if (f.size() >= 6 && f[0] == "0") model = true;
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
                if (n == D) return bad((long)li + 1, "more than the " + std::to_string(D) + " skews of the output layer");
                if (!skew_ok(v)) return bad((long)li + 1, "skew " + t + " of bin " + std::to_string(n) + " is not positive and finite");
                kappas[n++] = (float)v;
            }
        }
        if (n != D) return bad(last, std::to_string(n) + " skews, the output layer has " + std::to_string(D));
        return true;
    }
    int row = 0;
    for (size_t li = 0; li < lines.size(); li++) {
        const std::vector<std::string> f = fields(lines[li]);
        if (f.empty() || f[0][0] == '#') continue;
        if (row == D) return bad((long)li + 1, "more than the " + std::to_string(D) + " rows of the output layer");
        if (f.size() < 6)
            return bad((long)li + 1, "a row has the fields d p_plus p_minus alpha best_beta best_kappa ..., this one has " + std::to_string(f.size()));
        double v[6];
        for (int k = 0; k < 6; k++)
            if (!number(f[k], &v[k])) return bad((long)li + 1, "field " + std::to_string(k + 1) + " '" + f[k] + "' is not a number");
        if (v[0] != (double)row) return bad((long)li + 1, "row " + f[0] + " where row " + std::to_string(row) + " belongs");
        if (std::isnan(v[5])) {
            kappas[row] = fallback;
        } else {
            if (!skew_ok(v[5])) return bad((long)li + 1, "best_kappa " + f[5] + " of bin " + std::to_string(row) + " is not positive and finite");
            kappas[row] = (float)v[5];
        }
        row++;
    }
    if (row != D) return bad(last, std::to_string(row) + " rows, the output layer has " + std::to_string(D));
    return true;
}

}  // namespace mlggd_host
