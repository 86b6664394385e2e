// asymfile.h -- the trainer's opt-in fit of the asymmetric GGD error model (MLGGD_ASYMMODEL=FILE, read in train_options.cc): the
// text file written from the CV set's signed error statistics (mlggd_error_stats_signed over every CV chunk, added,
// then mlggd_asym_fit over the grid of MLGGD_ERRMODEL_BETAS).  The reader of that file for MLGGD_ASYMMETRY=FILE,
// parse_asymmetry (also behind mlggd_read_asymmetry), is in binfile.h with its two siblings.  Not in the reference: the
// 28-key command line and the log file do not change.
//
// The row layout is chosen so that the SAME file reads as a shape file through parse_shapefactors (binfile.h) as it
// is: '#' header lines with a '# shared_beta' among them, rows 0..D-1 in order, five or more numeric fields, field 5
// best_beta.  best_kappa is the next field:
//   d p_plus p_minus alpha_at_best best_beta best_kappa alpha_at_shared kappa_at_shared
// p_plus / p_minus are P+ / n and P- / n at the bin's best shape.  One fit then feeds
// MLGGD_SHAPEFACTORS=fit.txt MLGGD_ASYMMETRY=fit.txt in the next epoch.
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

}  // namespace mlggd_host
