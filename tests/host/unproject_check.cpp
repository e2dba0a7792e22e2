// unproject_check.cpp -- stand-alone host program over visgeom_amd/csrc/vg_unproject.hpp, compiled by tests/test_convert_cpu.py with
// the address and undefined-behaviour sanitizers.  Reads cases from standard input, one per line:
//     <model id> <K intrinsics> <n> <n pairs u v>
// (strtod's spellings: "nan", "inf") and prints, per pixel, one line "<ok> <raw ray x y z> <ok> <unit ray x y z>" with 17
// significant digits.  Exit status 1 for a line it cannot read.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vg_unproject.hpp"

namespace {

bool next_number(char *&s, double &v)
{
    char *end = nullptr;
    v = std::strtod(s, &end);
    if (end == s) return false;
    s = end;
    return true;
}

template <int MODEL>
void run(const double *intr, const std::vector<double> &uv)
{
    for (size_t i = 0; i + 1 < uv.size(); i += 2) {
        double X[3] = {0., 0., 0.}, U[3];
        const bool ok = vg::unproject<MODEL>(intr, uv[i], uv[i + 1], X);
        const bool oku = vg::unproject_unit<MODEL>(intr, uv[i], uv[i + 1], U);
        std::printf("%d %.17g %.17g %.17g %d %.17g %.17g %.17g\n", (int)ok, ok ? X[0] : 0., ok ? X[1] : 0., ok ? X[2] : 0., (int)oku, U[0], U[1],
                    U[2]);
    }
}

}  // namespace

int main()
{
    char *line = nullptr;
    size_t cap = 0;
    int status = 0;
    while (getline(&line, &cap, stdin) > 0) {
        char *s = line;
        double v;
        if (!next_number(s, v)) continue;   // an empty line
        const int model = (int)v, K = vg::num_intrinsics(model);
        std::vector<double> intr, uv;
        bool good = K > 0;
        for (int k = 0; good && k < K; k++) {
            good = next_number(s, v);
            intr.push_back(v);
        }
        double n = 0.;
        good = good && next_number(s, n) && n >= 0. && n <= 1e6;
        for (int k = 0; good && k < 2 * (int)n; k++) {
            good = next_number(s, v);
            uv.push_back(v);
        }
        if (!good || !vg::dispatch_model(model, vg::AllModels{}, [&](auto m) { run<decltype(m)::value>(intr.data(), uv); })) {
            std::fprintf(stderr, "unproject_check: cannot read \"%.60s\"\n", line);
            status = 1;
            break;
        }
    }
    std::free(line);
    return status;
}
