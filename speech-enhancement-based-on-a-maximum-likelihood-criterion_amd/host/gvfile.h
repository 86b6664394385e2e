// gvfile.h -- the trainer's opt-in global variance report (MLGGD_GVFILE=FILE, read in train_options.cc): the text file written
// from the CV set's output statistics (mlggd_output_stats over every CV chunk, added, then mlggd_gv_fit).  The reader of
// that file for the decoders' gv=FILE, parse_gv (also behind mlggd_read_gv), is in binfile.h with its two siblings.  Not
// in the reference: the 28-key command line, the weights file and the log file do not change.
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

// The fit of `sums` ([4][D], added over the CV chunks, n samples) as text: '#' header lines with n, D, shared_eta,
// gv_ref_shared and gv_est_shared, then one row per bin
//   d gv_ref gv_est eta
// the variances in %.17g and the factors in %.9g, so that both read back to their bits; a bin without a fit has eta
// nan.  Returns the shared factor (1 when no bin has a fit).
inline float write_gv_file(const std::string &path, int D, int64_t n, const std::vector<double> &sums) {
    std::vector<double> est(D), ref(D);
    std::vector<float> eta(D);
    std::vector<uint8_t> fitted(D);
    double est_s = 0.0, ref_s = 0.0;
    float eta_s = 1.0f;
    int32_t fit_s = 0;
    if (mlggd_gv_fit(D, n, sums.data(), est.data(), ref.data(), eta.data(), fitted.data(), &est_s, &ref_s, &eta_s,
                     &fit_s) != MLGGD_OK)
        throw std::runtime_error(std::string("mlggd_gv_fit failed: ") + mlggd_last_error());
    FILE *fp = fopen(path.c_str(), "w");
    if (!fp) throw std::runtime_error("MLGGD_GVFILE: cannot write " + path);
    fprintf(fp, "# global variance equalisation of the CV set: eta = sqrt(gv_ref / gv_est), normalised outputs and targets\n");
    fprintf(fp, "# n %lld\n# D %d\n", (long long)n, D);
    if (fit_s) fprintf(fp, "# shared_eta %.9g\n", (double)eta_s);
    else fprintf(fp, "# shared_eta nan\n");
    fprintf(fp, "# gv_ref_shared %.17g\n# gv_est_shared %.17g\n# d gv_ref gv_est eta\n", ref_s, est_s);
    for (int d = 0; d < D; d++) {
        if (fitted[d]) fprintf(fp, "%d %.17g %.17g %.9g\n", d, ref[d], est[d], (double)eta[d]);
        else fprintf(fp, "%d %.17g %.17g nan\n", d, ref[d], est[d]);
    }
    if (fclose(fp) != 0) throw std::runtime_error("MLGGD_GVFILE: cannot write " + path);
    return eta_s;
}

}  // namespace mlggd_host
