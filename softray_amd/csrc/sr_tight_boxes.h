// sr_tight_boxes.h -- the boxes of the camera- / light-ordered copies of the four-wide tree, fitted to the records their rays can hit
// (k_tight_level / k_tight_top, sr_lbvh.hip).  One text for the gfx950 kernels and for a host compiler
// (tests/cpp/tight_boxes_tests.cpp).
//
// k_facing_partition leaves every leaf slot of a copy a LIVE RUN: the records of the leaf that the copy's rays (from one camera origin /
// into one light ball) can hit at all.  The base tree's boxes bound all records.  The rule below re-makes a copy's boxes bottom-up from
// the live records alone:
//   * a leaf slot's box is the union of the boxes of the records of its live run (each the box a build would make for that triangle);
//     an empty run makes the slot absent (n = -1);
//   * an inner slot's box is the union of the present slots of the node it links to; a node without a present slot makes it absent,
//     so a subtree without a live record is never entered;
//   * links (c) never change, and neither does the base tree.
// Levels are the wide tree's node levels, 0 = the root's.  A depth cut-off L stops the rule L levels above the deepest: only the nodes
// of the lowest L levels are re-made, the slots of every node above them keep the base box (a superset) and stay present -- except
// that a leaf slot takes its live run at every level, as it always did.  L < 0 or L >= the number of levels: every level.
#pragma once
#include <math.h>
#include <stdint.h>

#include "sr_types.h"

namespace sr {

struct TightBox { float lo[3], hi[3]; };

SR_HOST_DEVICE inline TightBox tight_empty() {
    TightBox b;
    for (int a = 0; a < 3; ++a) { b.lo[a] = INFINITY; b.hi[a] = -INFINITY; }
    return b;
}
SR_HOST_DEVICE inline TightBox tight_union(const TightBox& x, const TightBox& y) {
    TightBox b;
    for (int a = 0; a < 3; ++a) { b.lo[a] = fminf(x.lo[a], y.lo[a]); b.hi[a] = fmaxf(x.hi[a], y.hi[a]); }
    return b;
}

// the first (topmost) level whose nodes are re-made under the depth cut-off `cut` in a tree of `num_levels` node levels
SR_HOST_DEVICE inline int tight_first_level(int num_levels, int cut) {
    return (cut < 0 || cut >= num_levels) ? 0 : num_levels - cut;
}

// A leaf slot (ch.n > 0) of the base tree -> the copy's slot for the live run (run_first, run_count) inside the leaf.  `tighten`: the
// slot's node lies at a level the rule re-makes; box_of(k) is the box of record k.  A run that does not lie inside the leaf is not a run
// of this tree: the slot is left as the base tree has it.
template <class BoxOf>
SR_HOST_DEVICE inline void tight_leaf_slot(Bvh4Child& ch, int run_first, int run_count, bool tighten, BoxOf box_of) {
    if (run_first < 0 || run_count > ch.n - run_first) return;
    if (run_count <= 0) { ch.c += run_first; ch.n = -1; return; }
    ch.c += run_first;
    ch.n = run_count;
    if (!tighten) return;
    TightBox b = box_of(ch.c);
    for (int k = 1; k < run_count; ++k) b = tight_union(b, box_of(ch.c + k));
    for (int a = 0; a < 3; ++a) { ch.lo[a] = b.lo[a]; ch.hi[a] = b.hi[a]; }
}

// An inner slot (ch.n == 0) of a node at a re-made level; `below` is the node it links to, in the copy, already re-made.
SR_HOST_DEVICE inline void tight_inner_slot(Bvh4Child& ch, const Bvh4Node& below) {
    TightBox b = tight_empty();
    bool any = false;
    for (int k = 0; k < 4; ++k) {
        if (below.ch[k].n < 0) continue;
        TightBox c;
        for (int a = 0; a < 3; ++a) { c.lo[a] = below.ch[k].lo[a]; c.hi[a] = below.ch[k].hi[a]; }
        b = tight_union(b, c);
        any = true;
    }
    if (!any) { ch.n = -1; return; }
    for (int a = 0; a < 3; ++a) { ch.lo[a] = b.lo[a]; ch.hi[a] = b.hi[a]; }
}

}  // namespace sr
