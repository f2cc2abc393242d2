// tight_boxes_tests.cpp -- the rule that fits the boxes of the ordered node copies to their live records (softray_amd/csrc/sr_tight_boxes.h, the
// text k_tight_level / k_tight_top compile) on small four-wide trees, compiled for the host with AddressSanitizer and
// UndefinedBehaviorSanitizer and run on the CPU as a program of its own.  The driver below is the device launcher's: levels deepest first,
// the nodes of a re-made level read the level below from the copy.
//
// usage: tight_boxes_tests [random trees]        exit 0 = every check holds
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../softray_amd/csrc/sr_tight_boxes.h"

using namespace sr;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

struct Run { int first, count; };
struct Tree {
    std::vector<Bvh4Node> nodes;          // level order: children after their parent, one level down
    std::vector<int> level_first;         // [levels + 1]
    std::vector<TightBox> rec;            // box of every record, exactly as many as the leaves name
    std::vector<Run> runs;                // per (node, slot)
    int levels() const { return (int)level_first.size() - 1; }
    int level_of(int node) const { int lv = 0; while (level_first[lv + 1] <= node) ++lv; return lv; }
};

static TightBox box_of_child(const Bvh4Child& c) { TightBox b; for (int a = 0; a < 3; ++a) { b.lo[a] = c.lo[a]; b.hi[a] = c.hi[a]; } return b; }
static void set_box(Bvh4Child& c, const TightBox& b) { for (int a = 0; a < 3; ++a) { c.lo[a] = b.lo[a]; c.hi[a] = b.hi[a]; } }
static bool same_box(const TightBox& x, const TightBox& y) { return std::memcmp(&x, &y, sizeof(TightBox)) == 0; }
static bool inside(const TightBox& in, const TightBox& out) {
    for (int a = 0; a < 3; ++a) if (!(out.lo[a] <= in.lo[a] && in.hi[a] <= out.hi[a])) return false;
    return true;
}
static Bvh4Child empty_child() { Bvh4Child c; for (int a = 0; a < 3; ++a) { c.lo[a] = 1.0f; c.hi[a] = -1.0f; } c.c = 0; c.n = -1; return c; }

// the base boxes: a leaf bounds ALL its records, an inner slot the present slots below it
static void base_boxes(Tree& t) {
    for (int i = (int)t.nodes.size() - 1; i >= 0; --i)
        for (int k = 0; k < 4; ++k) {
            Bvh4Child& c = t.nodes[i].ch[k];
            if (c.n < 0) continue;
            TightBox b = tight_empty();
            if (c.n > 0) for (int q = 0; q < c.n; ++q) b = tight_union(b, t.rec[(size_t)c.c + q]);
            else for (int j = 0; j < 4; ++j) if (t.nodes[c.c].ch[j].n >= 0) b = tight_union(b, box_of_child(t.nodes[c.c].ch[j]));
            set_box(c, b);
        }
}

// what tight_boxes_device does, one level at a time
static std::vector<Bvh4Node> tighten(const Tree& t, int cut) {
    std::vector<Bvh4Node> out(t.nodes.size());
    const int first_tight = tight_first_level(t.levels(), cut);
    for (int lv = t.levels() - 1; lv >= 0; --lv)
        for (int i = t.level_first[lv]; i < t.level_first[lv + 1]; ++i)
            for (int k = 0; k < 4; ++k) {
                Bvh4Child ch = t.nodes[i].ch[k];
                const bool on = lv >= first_tight;
                if (ch.n > 0) {
                    const Run r = t.runs[(size_t)i * 4 + k];
                    tight_leaf_slot(ch, r.first, r.count, on, [&](int q) { return t.rec.at((size_t)q); });
                } else if (ch.n == 0 && on) {
                    tight_inner_slot(ch, out[ch.c]);
                }
                out[i].ch[k] = ch;
            }
    return out;
}

// live records below (node, slot) of the BASE tree
static void live_below(const Tree& t, int node, int slot, std::vector<int>& live) {
    const Bvh4Child& c = t.nodes[node].ch[slot];
    if (c.n < 0) return;
    if (c.n > 0) { const Run r = t.runs[(size_t)node * 4 + slot]; for (int q = 0; q < r.count; ++q) live.push_back(c.c + r.first + q); return; }
    for (int j = 0; j < 4; ++j) live_below(t, c.c, j, live);
}

static long checked_slots = 0, absent_slots = 0;
static void check_tree(const Tree& t, int cut, const char* what) {
    const std::vector<Bvh4Node> out = tighten(t, cut);
    const int first_tight = tight_first_level(t.levels(), cut);
    for (int i = 0; i < (int)t.nodes.size(); ++i) {
        const int lv = t.level_of(i);
        for (int k = 0; k < 4; ++k) {
            const Bvh4Child &b = t.nodes[i].ch[k], &o = out[i].ch[k];
            ++checked_slots;
            if (b.n < 0) { CHECK(o.n < 0, "%s cut %d: node %d slot %d: an empty slot came to life", what, cut, i, k); continue; }
            std::vector<int> live;
            live_below(t, i, k, live);
            if (b.n == 0) CHECK(o.c == b.c, "%s cut %d: node %d slot %d: link changed", what, cut, i, k);
            if (b.n > 0) {                                            // the live run, at every level
                const Run r = t.runs[(size_t)i * 4 + k];
                CHECK(o.c == b.c + r.first && o.n == (r.count > 0 ? r.count : -1), "%s cut %d: node %d slot %d: run (%d, %d) -> c %d n %d", what, cut, i, k, r.first, r.count, o.c, o.n);
            }
            if (lv >= first_tight) {
                CHECK((o.n < 0) == live.empty(), "%s cut %d: node %d slot %d: absent %d, live records below %zu", what, cut, i, k, (int)(o.n < 0), live.size());
                if (o.n < 0) { ++absent_slots; continue; }
                TightBox u = tight_empty();
                for (int q : live) u = tight_union(u, t.rec[(size_t)q]);
                CHECK(same_box(box_of_child(o), u), "%s cut %d: node %d slot %d: not the union of the live records' boxes", what, cut, i, k);
            } else {
                if (b.n == 0) CHECK(o.n == 0, "%s cut %d: node %d slot %d: an inner slot above the cut-off went absent", what, cut, i, k);
                CHECK(same_box(box_of_child(o), box_of_child(b)), "%s cut %d: node %d slot %d: a box above the cut-off changed", what, cut, i, k);
                if (o.n < 0) { ++absent_slots; continue; }
            }
            for (int q : live) CHECK(inside(t.rec[(size_t)q], box_of_child(o)), "%s cut %d: node %d slot %d: live record %d sticks out", what, cut, i, k, q);
            CHECK(inside(box_of_child(o), box_of_child(b)), "%s cut %d: node %d slot %d: larger than the base box", what, cut, i, k);
        }
    }
}

// a tree from a description by levels: spec[lv][node][slot] = -1 empty, 0 inner (the next free node of the next level), n > 0 leaf of n records
typedef std::vector<std::vector<std::vector<int>>> Spec;
static Tree make_tree(const Spec& spec, std::mt19937& rng) {
    Tree t;
    std::uniform_real_distribution<float> pos(-1.0f, 1.0f), ext(0.0f, 0.2f);
    t.level_first.push_back(0);
    int next_node = 0;
    for (size_t lv = 0; lv < spec.size(); ++lv) {
        next_node += (int)spec[lv].size();
        int child = next_node;
        for (const auto& nd : spec[lv]) {
            Bvh4Node n;
            for (int k = 0; k < 4; ++k) {
                n.ch[k] = empty_child();
                const int v = k < (int)nd.size() ? nd[k] : -1;
                if (v == 0) { n.ch[k].n = 0; n.ch[k].c = child++; }
                if (v > 0) {
                    n.ch[k].n = v; n.ch[k].c = (int)t.rec.size();
                    for (int q = 0; q < v; ++q) {
                        TightBox b;
                        for (int a = 0; a < 3; ++a) { b.lo[a] = pos(rng); b.hi[a] = b.lo[a] + ext(rng); }
                        t.rec.push_back(b);
                    }
                }
            }
            t.nodes.push_back(n);
        }
        t.level_first.push_back(next_node);
    }
    t.runs.assign(t.nodes.size() * 4, Run{0, 0});
    base_boxes(t);
    return t;
}
static void whole_runs(Tree& t) { for (size_t i = 0; i < t.nodes.size(); ++i) for (int k = 0; k < 4; ++k) t.runs[i * 4 + k] = Run{0, t.nodes[i].ch[k].n > 0 ? t.nodes[i].ch[k].n : 0}; }
static void all_cuts(const Tree& t, const char* what) { for (int cut = -1; cut <= t.levels() + 1; ++cut) check_tree(t, cut, what); }

int main(int argc, char** argv) {
    const int random_trees = argc > 1 ? std::atoi(argv[1]) : 200;
    std::mt19937 rng(20240607u);
    CHECK(tight_first_level(5, -1) == 0 && tight_first_level(5, 0) == 5 && tight_first_level(5, 1) == 4 && tight_first_level(5, 5) == 0 && tight_first_level(5, 9) == 0, "cut-off levels");
    {   // every record live: the copy is the base tree, bit for bit
        Tree t = make_tree({{{0, 0, 3, -1}}, {{4, 0}, {2, 2, 2, 2}}, {{1}}}, rng);
        whole_runs(t);
        const std::vector<Bvh4Node> out = tighten(t, -1);
        CHECK(std::memcmp(out.data(), t.nodes.data(), out.size() * sizeof(Bvh4Node)) == 0, "all live: the copy differs from the base tree");
        all_cuts(t, "all live");
    }
    {   // a leaf with no live record, beside live ones
        Tree t = make_tree({{{0, 4, 4}}, {{3, 3, 3, 3}}}, rng);
        whole_runs(t);
        t.runs[1] = Run{2, 0};                                        // node 0 slot 1
        t.runs[4 + 2] = Run{0, 0};                                    // node 1 slot 2
        t.runs[4 + 0] = Run{1, 2};
        all_cuts(t, "empty leaf");
    }
    {   // a subtree with no live record: absent all the way up to the slot that links to it, and a root with nothing live at all
        Tree t = make_tree({{{0, 0, 2}}, {{0, 3}, {0, 0}}, {{4, 4}, {2}, {1, 1, 1, 1}}}, rng);
        whole_runs(t);
        for (int i : {1, 3}) for (int k = 0; k < 4; ++k) t.runs[(size_t)i * 4 + k].count = 0;      // everything below root slot 0
        all_cuts(t, "dead subtree");
        const std::vector<Bvh4Node> out = tighten(t, -1);
        CHECK(out[0].ch[0].n < 0 && out[0].ch[1].n == 0 && out[1].ch[0].n < 0, "dead subtree: root slot 0 should be absent");
        const std::vector<Bvh4Node> cut1 = tighten(t, 1);
        CHECK(cut1[0].ch[0].n == 0 && cut1[1].ch[0].n == 0, "dead subtree, cut-off 1: slots above the lowest level stay");
        for (Run& r : t.runs) r.count = 0;
        all_cuts(t, "nothing live");
        const std::vector<Bvh4Node> dead = tighten(t, -1);
        for (int k = 0; k < 4; ++k) CHECK(dead[0].ch[k].n < 0, "nothing live: root slot %d", k);
    }
    {   // nodes with one child, a chain
        Tree t = make_tree({{{0}}, {{0}}, {{0}}, {{4}}}, rng);
        whole_runs(t);
        t.runs[3 * 4] = Run{3, 1};
        all_cuts(t, "chain");
        const std::vector<Bvh4Node> out = tighten(t, -1);
        CHECK(same_box(box_of_child(out[0].ch[0]), t.rec[3]), "chain: the root's box is the one live record's");
    }
    {   // a run that does not lie in its leaf: the slot stays as the base tree has it
        Bvh4Child c = empty_child();
        c.c = 10; c.n = 3;
        Bvh4Child d = c;
        tight_leaf_slot(d, 2, 2, true, [&](int) { ++failures; return tight_empty(); });
        CHECK(std::memcmp(&c, &d, sizeof c) == 0, "a run outside its leaf changed the slot");
        d = c;
        tight_leaf_slot(d, -1, 1, true, [&](int) { ++failures; return tight_empty(); });
        CHECK(std::memcmp(&c, &d, sizeof c) == 0, "a run before its leaf changed the slot");
    }
    // random trees, random runs
    for (int it = 0; it < random_trees; ++it) {
        const int depth = 1 + (int)(rng() % 5);
        Spec spec;
        int wanted = 1;
        for (int lv = 0; lv < depth && wanted > 0; ++lv) {
            spec.emplace_back();
            int inner = 0;
            for (int i = 0; i < wanted; ++i) {
                std::vector<int> nd;
                const int slots = 1 + (int)(rng() % 4);
                for (int k = 0; k < slots; ++k) {
                    const unsigned r = rng() % 8;
                    if (r == 0) nd.push_back(-1);
                    else if (r < 4 && lv + 1 < depth && inner < 40) { nd.push_back(0); ++inner; }
                    else nd.push_back(1 + (int)(rng() % 5));
                }
                spec.back().push_back(nd);
            }
            wanted = inner;
        }
        Tree t = make_tree(spec, rng);
        const unsigned dead_share = rng() % 4;                       // 0: about half live ... 3: few live
        for (size_t i = 0; i < t.nodes.size(); ++i)
            for (int k = 0; k < 4; ++k) {
                const int n = t.nodes[i].ch[k].n;
                if (n <= 0) continue;
                const int first = (int)(rng() % (unsigned)(n + 1));
                int count = (int)(rng() % (unsigned)(n - first + 1));
                if (dead_share && rng() % (dead_share + 1)) count = 0;
                t.runs[i * 4 + k] = Run{first, count};
            }
        all_cuts(t, "random");
    }
    std::printf("TOTAL slots=%ld absent=%ld failures=%d\n", checked_slots, absent_slots, failures);
    return failures ? 1 : 0;
}
