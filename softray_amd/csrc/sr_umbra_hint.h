// sr_umbra_hint.h -- the per-tile umbra hint of the persistent packet shaft walk (k_shaft_pkt4, sr_pipeline.hip): one
// 32-bit word per 8x8-pixel tile that names the leaf whose triangle put lanes of the tile into umbra on the previous frame.  One text
// for the gfx950 kernel and for a host compiler (tests/cpp/umbra_hint_tests.cpp).
//
// The word names the light-live RUN of a leaf child as the light-ordered copy of the four-wide tree stores it -- first record cc, count
// cn -- and not one record: k_facing_partition permutes the records inside a leaf when the camera moves, the run starts at the leaf's
// first record whatever the camera does.  word = (cc << 4) | cn with 1 <= cn <= 15 and cc + cn <= nrec < 2^28; every other word means
// "no hint".  A word read from memory is only ever used through hint_unpack, which accepts it only if the whole run lies inside the
// frame's nrec records: a stale or uninitialised word costs a few triangle filters (each an exact umbra test) and can
// neither read out of bounds nor change a pixel.
#pragma once
#include <stdint.h>

#include "sr_types.h"

namespace sr {

constexpr uint32_t kHintAbsent = 0xFFFFFFFFu;        // decodes to cc + cn = 2^28 + 14 > nrec: never accepted
constexpr uint32_t kHintMaxRecords = 1u << 28;       // nrec at or above this: no hints at all

// the word of the run [cc, cc + cn), or kHintAbsent when the run has no word
SR_HOST_DEVICE inline uint32_t hint_pack(uint32_t cc, uint32_t cn) {
    return (cn >= 1u && cn <= 15u && cc < kHintMaxRecords) ? ((cc << 4) | cn) : kHintAbsent;
}

// true: `word` names a run inside [0, nrec), returned in cc / cn.  (cc < 2^28 and cn < 16: the sum cannot wrap)
SR_HOST_DEVICE inline bool hint_unpack(uint32_t word, uint32_t nrec, uint32_t& cc, uint32_t& cn) {
    cc = word >> 4;
    cn = word & 15u;
    return cn != 0u && nrec < kHintMaxRecords && cc + cn <= nrec;
}

}  // namespace sr
