// net_jump_tests.cpp -- the jump-ahead of System.Random (softray_amd/csrc/sr_host.cpp: net_random_window, net_jump_poly, net_jump_rows,
// net_jump_apply) against NetRandom itself, one draw after the other.  Host code only: compiled together with sr_host.cpp, with the
// address and undefined-behaviour sanitizers (tests/test_ao_points_model.py).
//
// usage: net_jump_tests [longest skip that is also drawn one after the other, default 20000]        exit 0 = every comparison holds
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../softray_amd/csrc/sr_host.h"

using namespace sr;

int main(int argc, char** argv) {
    const uint64_t longest = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 20000ull;
    const int32_t seeds[] = {1234567890, 0, 1, -1, INT32_MIN, 161803398, 161803399};
    const uint64_t skips[] = {0, 1, 33, 34, 54, 55, 56, 299, 300, 19200, 300ull << 17, 100000000ull};
    int bad = 0;
    for (int32_t seed : seeds) {
        int32_t w[kNetWindow];
        if (!net_random_window(seed, w)) { std::printf("seed %d: the first 55 outputs leave [0, 2^31 - 2]\n", seed); ++bad; continue; }
        for (uint64_t skip : skips) {
            if (skip > longest) continue;
            uint32_t c[kNetLag];
            int32_t out[kNetLag];
            net_jump_poly(skip, c);
            net_jump_apply(w, c, out);
            NetRandom r(seed);
            for (uint64_t i = 0; i < skip; ++i) (void)r.next();
            for (int i = 0; i < kNetLag; ++i)
                if (r.next() != out[i]) { ++bad; std::printf("seed %d skip %llu: value %d differs\n", seed, (unsigned long long)skip, i); break; }
        }
        // the rows of a stride are the polynomials of stride, stride + 1, ...
        static uint32_t rows[kNetLag * kNetLag];
        net_jump_rows(19200, rows);
        for (int i = 0; i < kNetLag; i += 9) {
            uint32_t c[kNetLag];
            net_jump_poly(19200 + (uint64_t)i, c);
            for (int j = 0; j < kNetLag; ++j)
                if (c[j] != rows[i * kNetLag + j]) { ++bad; std::printf("row %d of the stride differs\n", i); break; }
        }
        // beyond what can be drawn: consecutive windows overlap, and the recurrence holds across a window and the next one
        const uint64_t far = (1ull << 40) - 55;
        uint32_t c[kNetLag];
        int32_t a[kNetLag], b[kNetLag], d[kNetLag];
        net_jump_poly(far, c); net_jump_apply(w, c, a);
        net_jump_poly(far + 1, c); net_jump_apply(w, c, b);
        net_jump_poly(far + 55, c); net_jump_apply(w, c, d);
        for (int i = 0; i < 54; ++i)
            if (a[i + 1] != b[i]) { ++bad; std::printf("seed %d: windows at 2^40 - 55 and 2^40 - 54 do not overlap\n", seed); break; }
        for (int i = 0; i < 34; ++i) {
            int32_t e = a[i] - a[i + 21];
            if (e < 0) e += (int32_t)kNetPrime;
            if (e != d[i]) { ++bad; std::printf("seed %d: the recurrence fails at 2^40\n", seed); break; }
        }
    }
    std::printf("net_jump_tests: %d failures\n", bad);
    return bad != 0;
}
