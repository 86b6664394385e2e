// binfile.h -- the one reader of the host tools' per-bin model files: one positive, finite float per output bin from
// either
//   - a plain list: exactly D numbers separated by white space, any number per line ('#' lines are skipped), or
//   - a model file, the text a trainer report writes (errmodel.h, asymfile.h, gvfile.h): '#' header lines, then the
//     data rows 0..D-1 in order, of which ONE field is the bin's value.
// A file is taken for a model file when a '#' line comes before its first number, or when its first data line has the
// fields of a row and starts with the row number 0 (no list can start with 0: every value is positive).  What differs
// between the three models is a BinFile description and the few lines each reader has of its own: parse_shapefactors,
// parse_asymmetry and parse_gv below.  Every refusal is *err = "PATH line N: what is wrong" -- a wrong count (named at
// the file's last line, or line 1 of an empty file), a row out of order, a field that is no number, a value that is
// not positive and finite as a float -- and leaves the output unspecified.  No dependency on mlggd.h.
#pragma once
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace mlggd_host {

struct BinFile {
    const char *one, *many;   // the value in the messages: "shape", "shapes"
    int fields;               // a row needs this many numeric fields; the LAST of them, `column`, is the bin's value
    const char *column;       // "best_beta"
    const char *row_layout;   // the row as the "too few fields" message spells it
    const char *shared_key;   // "# KEY X" / "#KEY X" header line that is read, or nullptr: every '#' line is skipped
    bool nan_shared_counts;   // true: 'KEY nan' is a shared value like any other; false: a non-finite X is passed over
    bool nan_in_list;         // true: a 'nan' in a plain list marks a bin without a fit, as it does in a row
    bool unreadable_line_1;   // true: "PATH line 1: cannot read the file"; false: "cannot read PATH"
};

struct BinFileRead {
    bool model = false;           // a model file, not a plain list
    long last = 1;                // the line that count errors name: max(lines, 1)
    bool have_shared = false;     // a shared_key line was read ...
    double shared = std::nan(""); // ... and its value (the last one, when there are several)
};

inline bool binfile_bad(const std::string &path, long line, const std::string &what, std::string *err) {
    *err = path + " line " + std::to_string(line) + ": " + what;
    return false;
}

// The D values of `path` into out[]; a bin without a fit ('nan' in a row's column, or in a list where the description
// allows it) is left NaN for the caller to fill, which no accepted value is.
inline bool read_binfile(const BinFile &m, const std::string &path, int D, float *out, BinFileRead *got, std::string *err) {
    auto bad = [&](long line, const std::string &what) { return binfile_bad(path, line, what, err); };
    FILE *fp = fopen(path.c_str(), "r");
    if (!fp) {
        if (m.unreadable_line_1) return bad(1, "cannot read the file");
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
    auto value_ok = [](double v) { return (float)v > 0.0f && std::isfinite((float)v); };
    const std::string sD = std::to_string(D), one = m.one, many = m.many;
    // which of the two formats
    for (const std::string &l : lines) {
        const std::vector<std::string> f = fields(l);
        if (f.empty()) continue;
        if (f[0][0] == '#') got->model = true;
        else if ((int)f.size() >= m.fields && f[0] == "0") got->model = true;
        break;
    }
    got->last = (long)lines.size() > 0 ? (long)lines.size() : 1;
    if (!got->model) {
        int n = 0;
        for (size_t li = 0; li < lines.size(); li++) {
            const std::vector<std::string> f = fields(lines[li]);
            if (!f.empty() && f[0][0] == '#') continue;
            for (const std::string &t : f) {
                double v;
                if (!number(t, &v)) return bad((long)li + 1, "'" + t + "' is not a number");
                if (n == D) return bad((long)li + 1, "more than the " + sD + " " + many + " of the output layer");
                if (!(m.nan_in_list && std::isnan(v)) && !value_ok(v))
                    return bad((long)li + 1, one + " " + t + " of bin " + std::to_string(n) + " is not positive and finite");
                out[n++] = (float)v;
            }
        }
        if (n != D) return bad(got->last, std::to_string(n) + " " + many + ", the output layer has " + sD);
        return true;
    }
    const std::string key = m.shared_key ? m.shared_key : "";
    const int col = m.fields - 1;
    int row = 0;
    for (size_t li = 0; li < lines.size(); li++) {
        const std::vector<std::string> f = fields(lines[li]);
        if (f.empty()) continue;
        if (f[0][0] == '#') {
            const size_t k = f[0] == "#" ? 1 : 0;  // "# KEY X" or "#KEY X"
            if (m.shared_key && f.size() > k + 1 && (f[k] == key || f[k] == "#" + key)) {
                double v;
                if (!number(f[k + 1], &v)) return bad((long)li + 1, key + " '" + f[k + 1] + "' is not a number");
                if (m.nan_shared_counts || std::isfinite(v)) {
                    if (!std::isnan(v) && !value_ok(v)) return bad((long)li + 1, key + " " + f[k + 1] + " is not positive and finite");
                    got->shared = v;
                    got->have_shared = true;
                }
            }
            continue;
        }
        if (row == D) return bad((long)li + 1, "more than the " + sD + " rows of the output layer");
        if ((int)f.size() < m.fields)
            return bad((long)li + 1, std::string("a row has the fields ") + m.row_layout + ", this one has " + std::to_string(f.size()));
        double v = 0.0, d = 0.0;
        for (int k = 0; k < m.fields; k++) {
            if (!number(f[k], &v)) return bad((long)li + 1, "field " + std::to_string(k + 1) + " '" + f[k] + "' is not a number");
            if (k == 0) d = v;
        }
        if (d != (double)row) return bad((long)li + 1, "row " + f[0] + " where row " + std::to_string(row) + " belongs");
        if (!std::isnan(v) && !value_ok(v))
            return bad((long)li + 1, std::string(m.column) + " " + f[col] + " of bin " + std::to_string(row) + " is not positive and finite");
        out[row++] = (float)v;
    }
    if (row != D) return bad(got->last, std::to_string(row) + " rows, the output layer has " + sD);
    return true;
}

inline void binfile_fill_unfit(int D, float *out, float with) {
    for (int d = 0; d < D; d++)
        if (std::isnan(out[d])) out[d] = with;
}

// MLGGD_SHAPEFACTORS=FILE, mlggd_read_shapefactors: one shape per bin from a list, or from field 5, best_beta, of the
// file write_error_model (errmodel.h) or write_asym_model (asymfile.h) writes.  A finite '# shared_beta' is remembered;
// a bin without a fit takes it, or `fallback` when the file has none.  A 'nan' in a list is refused.
inline bool parse_shapefactors(const std::string &path, int D, float fallback, float *betas, std::string *err) {
    static const BinFile m = {"shape", "shapes", 5, "best_beta", "d mean var kurt best_beta ...", "shared_beta", false, false, false};
    BinFileRead got;
    if (!read_binfile(m, path, D, betas, &got, err)) return false;
    binfile_fill_unfit(D, betas, got.have_shared ? (float)got.shared : fallback);
    return true;
}

// MLGGD_ASYMMETRY=FILE, mlggd_read_asymmetry: one skew per bin from a list, or from field 6, best_kappa, of the file
// write_asym_model writes.  No header line is read; a bin without a fit takes `fallback`.  A 'nan' in a list is refused.
inline bool parse_asymmetry(const std::string &path, int D, float fallback, float *kappas, std::string *err) {
    static const BinFile m = {"skew", "skews", 6, "best_kappa", "d p_plus p_minus alpha best_beta best_kappa ...", nullptr, false, false, false};
    BinFileRead got;
    if (!read_binfile(m, path, D, kappas, &got, err)) return false;
    binfile_fill_unfit(D, kappas, fallback);
    return true;
}

// gv=FILE of the decoders, mlggd_read_gv: one factor per bin from a list, or from field 4, eta, of the file
// write_gv_file (gvfile.h) writes.  A 'nan', in a row or in a list, is a bin without a fit and takes 1.  shared: every
// bin takes the file's '# shared_eta' instead (nan: 1); a plain list and a file without that line have none, which is
// an error.  A file that cannot be read is reported at its line 1.
inline bool parse_gv(const std::string &path, int D, bool shared, float *eta, std::string *err) {
    static const BinFile m = {"factor", "factors", 4, "eta", "d gv_ref gv_est eta", "shared_eta", true, true, true};
    BinFileRead got;
    if (!read_binfile(m, path, D, eta, &got, err)) return false;
    binfile_fill_unfit(D, eta, 1.0f);
    if (!shared) return true;
    if (!got.model) return binfile_bad(path, got.last, "a plain list has no shared factor", err);
    if (!got.have_shared) return binfile_bad(path, got.last, "the file has no '# shared_eta' line", err);
    for (int d = 0; d < D; d++) eta[d] = std::isnan(got.shared) ? 1.0f : (float)got.shared;
    return true;
}

}  // namespace mlggd_host
