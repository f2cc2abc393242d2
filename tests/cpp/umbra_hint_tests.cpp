// umbra_hint_tests.cpp -- the hint word of the persistent packet shaft walk (softray_amd/csrc/sr_umbra_hint.h, the text k_shaft_pkt4
// compiles): pack, unpack and the bounds rule against a scalar model written from the rule's words, compiled for the host and run on the
// CPU.  A word that hint_unpack accepts must name a run of 1..15 records that lies inside [0, nrec); every accepted run is walked over
// an array of exactly nrec bytes, so a build with -fsanitize=address,undefined stops at the first index the rule lets through.
//
// usage: umbra_hint_tests [random words]        exit 0 = every check holds
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../softray_amd/csrc/sr_umbra_hint.h"

namespace {

int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

// the rule as DESIGN.md states it, in 64-bit arithmetic: word = (cc << 4) | cn, 1 <= cn <= 15, cc + cn <= nrec < 2^28
bool model_accepts(uint32_t word, uint64_t nrec, uint64_t& cc, uint64_t& cn) {
    cc = (uint64_t)word >> 4;
    cn = (uint64_t)word & 15u;
    return cn >= 1 && cn <= 15 && nrec < (1ull << 28) && cc + cn <= nrec;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rng() {                                        // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// what the kernel does with a word: every record of an accepted run is read
unsigned long touch(const std::vector<uint8_t>& records, uint32_t word) {
    uint32_t cc, cn;
    unsigned long sum = 0;
    if (sr::hint_unpack(word, (uint32_t)records.size(), cc, cn))
        for (uint32_t q = 0; q < cn; ++q) sum += records[(size_t)cc + q] + 1u;
    return sum;
}

}  // namespace

int main(int argc, char** argv) {
    const long random_words = argc > 1 ? atol(argv[1]) : 200000;
    uint32_t cc = 0, cn = 0;
    // ---- pack: a run has a word exactly when 1 <= cn <= 15 and cc < 2^28 ----
    CHECK(sr::hint_pack(0u, 0u) == sr::kHintAbsent);                   // cn = 0
    CHECK(sr::hint_pack(7u, 16u) == sr::kHintAbsent);                  // cn = 16
    CHECK(sr::hint_pack(1u << 28, 1u) == sr::kHintAbsent);
    CHECK(sr::hint_pack(0xFFFFFFFFu, 3u) == sr::kHintAbsent);
    CHECK(sr::hint_pack(5u, 1u) == ((5u << 4) | 1u));
    CHECK(sr::hint_pack((1u << 28) - 1u, 15u) == 0xFFFFFFFFu);         // the only run whose word IS the absent word: beyond every nrec
    // ---- unpack: cn = 0 and (through pack) cn = 16 ----
    CHECK(!sr::hint_unpack(40u << 4, 1000u, cc, cn));                  // cn = 0
    CHECK(!sr::hint_unpack(sr::hint_pack(40u, 16u), 1000u, cc, cn));   // cn = 16 has no word
    // ---- the end of the records: cc + cn = nrec is the last run, nrec + 1 is outside ----
    for (uint32_t n = 1; n <= 15; ++n) {
        const uint32_t nrec = 1000u;
        CHECK(sr::hint_unpack(sr::hint_pack(nrec - n, n), nrec, cc, cn) && cc == nrec - n && cn == n);
        CHECK(!sr::hint_unpack(sr::hint_pack(nrec - n + 1u, n), nrec, cc, cn));
        CHECK(!sr::hint_unpack(sr::hint_pack(nrec, n), nrec, cc, cn));
    }
    CHECK(sr::hint_unpack(sr::hint_pack(0u, 1u), 1u, cc, cn) && cc == 0u && cn == 1u);
    CHECK(!sr::hint_unpack(sr::hint_pack(0u, 1u), 0u, cc, cn));        // no records: nothing is accepted
    CHECK(!sr::hint_unpack(sr::hint_pack(0u, 2u), 1u, cc, cn));
    // ---- the absent word, for every nrec the kernel can be given ----
    for (uint64_t nrec : {0ull, 1ull, 15ull, 1000ull, (1ull << 28) - 1ull, 1ull << 28, (1ull << 28) + 14ull, (1ull << 28) + 15ull, 0x7fffff00ull, 0xFFFFFFFFull})
        CHECK(!sr::hint_unpack(sr::kHintAbsent, (uint32_t)nrec, cc, cn));
    // ---- nrec >= 2^28: no word at all ----
    CHECK(!sr::hint_unpack(sr::hint_pack(3u, 2u), 1u << 28, cc, cn));
    CHECK(sr::hint_unpack(sr::hint_pack(3u, 2u), (1u << 28) - 1u, cc, cn));
    // ---- random words against the scalar model, and the accepted runs against a records array of exactly nrec bytes ----
    long accepted = 0, rejected = 0;
    for (uint32_t nrec : {0u, 1u, 7u, 16u, 600u, 6002u, 1000000u}) {
        std::vector<uint8_t> records(nrec, 1);
        unsigned long sink = 0;
        for (long i = 0; i < random_words; ++i) {
            const uint64_t r = rng();
            uint32_t w = (uint32_t)r;
            switch ((r >> 32) & 3u) {                                    // a third of the words near the end of the records, where the rule decides
                case 0: w = (uint32_t)((((uint64_t)nrec + (r >> 40) % 40u) - 20u) << 4) | (w & 15u); break;
                case 1: w = (uint32_t)(((r >> 40) % ((uint64_t)nrec + 1u)) << 4) | (w & 15u); break;
                default: break;
            }
            uint64_t mc, mn;
            const bool want = model_accepts(w, nrec, mc, mn);
            const bool got = sr::hint_unpack(w, nrec, cc, cn);
            CHECK(got == want);
            if (got) { CHECK(cc == mc && cn == mn && sr::hint_pack(cc, cn) == w); ++accepted; } else ++rejected;
            sink += touch(records, w);
            if (failures > 20) { printf("too many failures\n"); return 1; }
        }
        if (sink == 0xFFFFFFFFFFFFFFFFul) printf(" ");                   // (keeps the reads)
    }
    printf("TOTAL accepted=%ld rejected=%ld failures=%d\n", accepted, rejected, failures);
    return failures == 0 && accepted > 0 && rejected > 0 ? 0 : 1;
}
