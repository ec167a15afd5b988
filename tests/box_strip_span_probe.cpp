// Host program for tests/test_box_strip_span_host.py: nt_box_strip_span (ntracer_amd/csrc/nt_box_span.hpp) of every camera read
// from standard input, one a line -- "n" and then origin, right, up, forward, n numbers each ("nan", "inf" as strtof reads
// them) -- printed as "lo hi" with nine digits, one line a camera.  With "--time n reps" it times the function alone on `reps`
// cameras of a rotation around the cube and prints the microseconds a camera.
// The header is host-compilable on its own (g++ -std=c++17 -I ntracer_amd/csrc).
#include <chrono>
#include <cmath>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "nt_box_span.hpp"

static int time_it(int n, int reps) {
    if (n < 3 || n > 64 || reps < 1) return 2;
    std::vector<float> o(n), r(n), u(n), f(n);
    double sum = 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < reps; ++k) {
        // a camera that circles the cube in the plane of axes 0 and 2 at distance 5, tilted a little into every other axis
        const double ang = 0.1 + 6.0 * k / reps;
        for (int j = 0; j < n; ++j) { o[j] = 0.05f * (float)j; r[j] = 0.0f; u[j] = 0.0f; f[j] = 0.01f * (float)j; }
        o[0] = (float)(-5.0 * std::sin(ang)); o[2] = (float)(-5.0 * std::cos(ang));
        f[0] = (float)std::sin(ang); f[2] = (float)std::cos(ang);
        r[0] = (float)std::cos(ang); r[2] = (float)-std::sin(ang);
        u[1] = 1.0f;
        const NtBoxSpan s = nt_box_strip_span(n, o.data(), r.data(), u.data(), f.data());
        sum += std::isfinite(s.lo) ? s.lo : 0.0;
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    printf("%d %.3f %g\n", n, us / reps, sum);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && strcmp(argv[1], "--time") == 0) return time_it(atoi(argv[2]), atoi(argv[3]));
    if (argc != 1) {
        fprintf(stderr, "usage: %s < cameras   |   %s --time n reps\n", argv[0], argv[0]);
        return 2;
    }
    std::string line;
    int ch;
    while (true) {
        line.clear();
        while ((ch = getchar()) != EOF && ch != '\n') line.push_back((char)ch);
        if (line.empty() && ch == EOF) break;
        if (line.empty()) continue;
        std::vector<float> v;
        const char *p = line.c_str();
        char *end = nullptr;
        const long n = strtol(p, &end, 10);
        p = end;
        while (true) {
            const float x = strtof(p, &end);
            if (end == p) break;
            v.push_back(x);
            p = end;
        }
        if (n < 1 || n > 64 || v.size() != (size_t)(4 * n)) {
            fprintf(stderr, "bad camera line: %s\n", line.c_str());
            return 2;
        }
        const NtBoxSpan s = nt_box_strip_span((int)n, v.data(), v.data() + n, v.data() + 2 * n, v.data() + 3 * n);
        printf("%.9g %.9g\n", (double)s.lo, (double)s.hi);
        if (ch == EOF) break;
    }
    return 0;
}
