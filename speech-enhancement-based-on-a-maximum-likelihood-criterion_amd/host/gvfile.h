// gvfile.h -- the trainer's opt-in global variance report (MLGGD_GVFILE=FILE, bptrain_main.cc): the text file written
// from the CV set's output statistics (mlggd_output_stats over every CV chunk, added, then mlggd_gv_fit), and the reader
// of that file for the decoders' gv=FILE (parse_gv, also behind mlggd_read_gv).  Not in the reference: the 28-key
// command line, the weights file and the log file do not change.
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

// The way back (gv=FILE of the decoders, mlggd_read_gv): one factor per output bin from either
//   - a plain list: exactly D numbers separated by white space, any number per line, or
//   - the file write_gv_file writes: '#' lines are skipped ('# shared_eta X' is remembered), the data rows must be rows
//     0..D-1 in order and field 4 of row d, eta, is bin d's factor.
// A 'nan' marks a bin without a fit and takes 1.  shared: every bin takes the file's shared_eta (nan: 1); a plain list
// has none, which is an error.  A file is taken for the trainer's when a '#' line comes before its first number, or
// when its first data line has four or more fields and starts with the row number 0 (no list can start with 0: every
// factor is positive).  Returns false with *err = "PATH line N: what is wrong" on a file that cannot be read (line 1), a
// wrong count, a row out of order, a field that is no number and a factor that is not positive and finite; eta is then
// unspecified.
inline bool parse_gv(const std::string &path, int D, bool shared, float *eta, std::string *err) {
    auto bad = [&](long line, const std::string &what) {
        *err = path + " line " + std::to_string(line) + ": " + what;
        return false;
    };
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
    auto eta_ok = [](double v) { return (float)v > 0.0f && std::isfinite((float)v); };
    bool model = false;
    for (const std::string &l : lines) {
        const std::vector<std::string> f = fields(l);
        if (f.empty()) continue;
        if (f[0][0] == '#') model = true;
        else if (f.size() >= 4 && f[0] == "0") model = true;
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
                if (n == D) return bad((long)li + 1, "more than the " + std::to_string(D) + " factors of the output layer");
                if (std::isnan(v)) v = 1.0;
                if (!eta_ok(v)) return bad((long)li + 1, "factor " + t + " of bin " + std::to_string(n) + " is not positive and finite");
                eta[n++] = (float)v;
            }
        }
        if (n != D) return bad(last, std::to_string(n) + " factors, the output layer has " + std::to_string(D));
        if (shared) return bad(last, "a plain list has no shared factor");
        return true;
    }
    double shared_eta = std::nan("");
    bool have_shared = false;
    int row = 0;
    for (size_t li = 0; li < lines.size(); li++) {
        const std::vector<std::string> f = fields(lines[li]);
        if (f.empty()) continue;
        if (f[0][0] == '#') {
            const size_t k = f[0] == "#" ? 1 : 0;  // "# shared_eta X" or "#shared_eta X"
            if (f.size() > k + 1 && (f[k] == "shared_eta" || f[k] == "#shared_eta")) {
                double v;
                if (!number(f[k + 1], &v)) return bad((long)li + 1, "shared_eta '" + f[k + 1] + "' is not a number");
                if (!std::isnan(v) && !eta_ok(v)) return bad((long)li + 1, "shared_eta " + f[k + 1] + " is not positive and finite");
                shared_eta = v;
                have_shared = true;
            }
            continue;
        }
        if (row == D) return bad((long)li + 1, "more than the " + std::to_string(D) + " rows of the output layer");
        if (f.size() < 4) return bad((long)li + 1, "a row has the fields d gv_ref gv_est eta, this one has " + std::to_string(f.size()));
        double v[4];
        for (int k = 0; k < 4; k++)
            if (!number(f[k], &v[k])) return bad((long)li + 1, "field " + std::to_string(k + 1) + " '" + f[k] + "' is not a number");
        if (v[0] != (double)row) return bad((long)li + 1, "row " + f[0] + " where row " + std::to_string(row) + " belongs");
        if (std::isnan(v[3])) v[3] = 1.0;
        if (!eta_ok(v[3])) return bad((long)li + 1, "eta " + f[3] + " of bin " + std::to_string(row) + " is not positive and finite");
        eta[row++] = (float)v[3];
    }
    if (row != D) return bad(last, std::to_string(row) + " rows, the output layer has " + std::to_string(D));
    if (shared) {
        if (!have_shared) return bad(last, "the file has no '# shared_eta' line");
        for (int d = 0; d < D; d++) eta[d] = std::isnan(shared_eta) ? 1.0f : (float)shared_eta;
    }
    return true;
}

}  // namespace mlggd_host
