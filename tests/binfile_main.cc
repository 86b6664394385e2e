// binfile_main.cc -- the three per-bin model-file readers of the host tools (parse_shapefactors, parse_asymmetry and
// parse_gv; host/errmodel.h, host/asymfile.h, host/gvfile.h) as a stand-alone program for AddressSanitizer + UBSan;
// driven by tests/test_binfile_golden.py, which compares its output with tests/golden/binfile_cases.json line for line.
//
//   binfile_main DIR CASES
//
// changes into DIR (so that the messages name the files as the case list does) and reads CASES, one case per line:
//   READER FILE D VALUE      READER shape | asym | gv;  VALUE the fallback of shape / asym, 0 or 1 (shared) of gv
// For each it prints one JSON line: the case, the return value, the whole error text, and -- when the reader returned
// true -- the D floats as hex bit patterns (after a refusal they are unspecified and are not printed).  The output
// array is a heap array of exactly D floats.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "asymfile.h"
#include "errmodel.h"
#include "gvfile.h"

static std::string json(const std::string &s) {
    std::string o = "\"";
    char u[8];
    for (unsigned char c : s) {
        if (c == '"' || c == '\\') {
            o += '\\';
            o += (char)c;
        } else if (c < 0x20 || c >= 0x7f) {
            snprintf(u, sizeof u, "\\u%04x", c);
            o += u;
        } else {
            o += (char)c;
        }
    }
    return o + "\"";
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: binfile_main DIR CASES\n");
        return 2;
    }
    std::ifstream cases(argv[2]);
    if (!cases || chdir(argv[1]) != 0) {
        fprintf(stderr, "binfile_main: cannot read %s or enter %s\n", argv[2], argv[1]);
        return 2;
    }
    std::string line;
    while (std::getline(cases, line)) {
        std::istringstream is(line);
        std::string reader, file;
        int D = 0;
        float value = 0.0f;
        if (!(is >> reader >> file >> D >> value) || D < 1) {
            fprintf(stderr, "binfile_main: bad case '%s'\n", line.c_str());
            return 2;
        }
        std::vector<float> out((size_t)D, -7.0f);
        std::string err;
        bool ok;
        if (reader == "shape") ok = mlggd_host::parse_shapefactors(file, D, value, out.data(), &err);
        else if (reader == "asym") ok = mlggd_host::parse_asymmetry(file, D, value, out.data(), &err);
        else if (reader == "gv") ok = mlggd_host::parse_gv(file, D, value != 0.0f, out.data(), &err);
        else {
            fprintf(stderr, "binfile_main: unknown reader '%s'\n", reader.c_str());
            return 2;
        }
        printf("{\"reader\": %s, \"file\": %s, \"D\": %d, \"value\": %.9g, \"ok\": %s, \"err\": %s, \"bits\": [",
               json(reader).c_str(), json(file).c_str(), D, (double)value, ok ? "true" : "false", json(err).c_str());
        for (int d = 0; ok && d < D; d++) {
            uint32_t u;
            memcpy(&u, &out[d], 4);
            printf("%s\"%08x\"", d ? ", " : "", u);
        }
        printf("]}\n");
    }
    return 0;
}
