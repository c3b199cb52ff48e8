// tests/csrc/rows_norm_check.cpp — image_matching_amd/csrc/rows_norm.h on the host, driven by tests/test_rows_norm_host.py, which holds
// the expectations (numpy's conversions, the oracle's hyo_normalize).  Compiled with g++ -O2 -ffp-contract=off.
//   rows_norm_check f16  OUT          the 65536 binary16 patterns widened, as doubles
//   rows_norm_check bf16 OUT          the 65536 bfloat16 patterns widened
//   rows_norm_check f32  IN OUT       the binary32 patterns of IN (uint32) widened
//   rows_norm_check norm DIM IN OUT   every row of IN (doubles [n][DIM]) normalised
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rows_norm.h"

template <typename T>
static std::vector<T> read_all(const char *path) {
    std::vector<T> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(T));
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
    fclose(f);
    return v;
}
static int write_all(const char *path, const std::vector<double> &v) {
    FILE *f = fopen(path, "wb");
    if (!f) return 1;
    const size_t n = fwrite(v.data(), sizeof(double), v.size(), f);
    fclose(f);
    return n == v.size() ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const char *mode = argv[1];
    std::vector<double> out;
    if ((!strcmp(mode, "f16") || !strcmp(mode, "bf16")) && argc == 3) {
        out.resize(65536);
        for (unsigned b = 0; b < 65536; b++) out[b] = mode[0] == 'f' ? rn_widen_f16_bits((unsigned short)b) : rn_widen_bf16_bits((unsigned short)b);
        return write_all(argv[2], out);
    }
    if (!strcmp(mode, "f32") && argc == 4) {
        const std::vector<unsigned> in = read_all<unsigned>(argv[2]);
        for (unsigned b : in) out.push_back(rn_widen_f32_bits(b));
        return in.empty() ? 3 : write_all(argv[3], out);
    }
    if (!strcmp(mode, "norm") && argc == 5) {
        const int dim = atoi(argv[2]);
        out = read_all<double>(argv[3]);
        if (dim < 1 || out.empty() || out.size() % (size_t)dim) return 3;
        for (size_t r = 0; r < out.size() / (size_t)dim; r++) rn_normalise_row(out.data() + r * (size_t)dim, dim);
        return write_all(argv[4], out);
    }
    return 2;
}
