// errmodel.h -- the trainer's opt-in error-model report (MLGGD_ERRMODEL=FILE, read in train_options.cc): the shape grid of
// MLGGD_ERRMODEL_BETAS and the text file written from the CV set's error statistics (mlggd_error_stats over every CV
// chunk, added, then mlggd_ggd_fit).  The reader of that file for MLGGD_SHAPEFACTORS=FILE, parse_shapefactors (also
// behind mlggd_read_shapefactors), is in binfile.h with its two siblings.  Not in the reference: the 28-key command
// line and the log file do not change.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mlggd.h"
#include "binfile.h"

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

}  // namespace mlggd_host
