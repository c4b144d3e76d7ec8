// frontier_check.cpp -- the split loops' shared greedy step (SplitFrontier, through lq_replay) against the whole-frontier loop it
// replaced (lq_replay_plain), over random candidate trees.  Host code only: test_split_frontier.py builds this with
// -fsanitize=address,undefined and runs it.  Exit status 0 and a line of counts: every tree agreed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "split_frontier.h"

using namespace pamd;

namespace {
constexpr double kDelta = 1e-16;                       // math/misc.h:5

struct Rng {                                           // splitmix64: the same trees everywhere
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ULL); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; return z ^ (z >> 31); }
    unsigned below(unsigned n) { return (unsigned)(next() % n); }
    double unit() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

enum Values { kContinuous, kTies, kTiny };
struct Shape { Values values; unsigned unknown_pct, nosplit_pct; };

double draw(Rng &r, Values v) {
    static const double tiny[] = {0.0, 1e-17, 5e-17, 9.9e-17, 1e-16, 2e-16, 1e-15};   // around DELTA: the stop is hit
    if (v == kTies) return 0.25 * (1 + r.below(4));                  // four values: exact ties everywhere, within and across blocks
    if (v == kTiny && r.below(3) == 0) return tiny[r.below(7)];
    return r.unit();
}

// nodes 0 .. first_base-1 are not part of the tree (poisoned: a step that reads them commits nonsense), then the base clusters, then
// the children in consecutive pairs.  A known node is a split (its benefit, its left child) or never splits (0, no child); an
// undecided one carries a bound.  The table ends after ~2K splits: what is left becomes a leaf.
std::vector<LqRec> make_tree(Rng &r, size_t K, int kbase, int first_base, const Shape &sh) {
    std::vector<LqRec> t;
    for (int i = 0; i < first_base; i++) t.push_back(LqRec{1e300, -1, 1});
    for (int i = 0; i < kbase; i++) t.push_back(LqRec{0.0, -1, 0});
    const size_t cap = (size_t)first_base + kbase + 2 * (K + 4 + r.below(8));
    for (size_t i = (size_t)first_base; i < t.size(); i++) {
        const unsigned p = r.below(100);
        const double v = draw(r, sh.values);
        if (p < sh.unknown_pct) t[i] = LqRec{v, -1, 0};
        else if (p < sh.unknown_pct + sh.nosplit_pct || t.size() + 2 > cap) t[i] = LqRec{0.0, -1, 1};
        else {
            t[i] = LqRec{v, (int)t.size(), 1};
            t.push_back(LqRec{0.0, -1, 0}); t.push_back(LqRec{0.0, -1, 0});
        }
    }
    return t;
}

bool same_commits(const std::vector<LqCommit> &a, const std::vector<LqCommit> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].row != b[i].row || a[i].node != b[i].node || a[i].new_row != b[i].new_row || a[i].left != b[i].left) return false;
    return true;
}

struct Counts { long trees = 0, full = 0, stopped = 0, blocked = 0, sabotaged = 0; };

// both loops over one tree, with and without the sabotaged step; false (and a line on stderr) if they differ anywhere
bool check_tree(const std::vector<LqRec> &t, int kbase, int first_base, size_t K, Counts &c, const char *what) {
    std::vector<int> honest;
    for (int fault = 0; fault <= 2; fault += 2) {
        LqReplay a, b;
        const bool ra = lq_replay(t.data(), kbase, first_base, K, kDelta, fault, a);
        const bool rb = lq_replay_plain(t.data(), kbase, first_base, K, kDelta, fault, b);
        if (ra != rb || a.result != b.result || !same_commits(a.commits, b.commits) || a.stopped_early != b.stopped_early) {
            fprintf(stderr, "frontier_check: %s: K %zu, kbase %d, first_base %d, fault %d: blocked form %d / %zu rows / %zu commits / stopped %d, plain %d / %zu / %zu / %d\n",
                    what, K, kbase, first_base, fault, (int)ra, a.result.size(), a.commits.size(), (int)a.stopped_early, (int)rb, b.result.size(),
                    b.commits.size(), (int)b.stopped_early);
            return false;
        }
        if (fault == 0) {
            honest = a.result;
            c.trees++;
            if (!ra) c.blocked++; else if (a.stopped_early) c.stopped++; else c.full++;
        } else if (a.result != honest) c.sabotaged++;
    }
    return true;
}

// Every known value equal, K = 33, one base cluster: the frontier grows to 32 rows over three blocks, all tied.  The first maximum
// is row 0 at every step (its right child takes its place and ties again), so every commit is of row 0.
bool check_tie_across_blocks(Counts &c) {
    const size_t K = 33;
    std::vector<LqRec> t;
    t.push_back(LqRec{1.0, 1, 1});
    for (size_t i = 0; i < 2 * K; i++) {
        const int id = (int)t.size();
        t.push_back(LqRec{1.0, id + 2, 1}); t.push_back(LqRec{1.0, id + 2, 1});   // both children of a pair split into the next pair: a chain is enough
    }
    t.push_back(LqRec{0.0, -1, 1}); t.push_back(LqRec{0.0, -1, 1});   // (the chain's end, never reached)
    if (!check_tree(t, 1, 0, K, c, "all tied")) return false;
    LqReplay a;
    if (!lq_replay(t.data(), 1, 0, K, kDelta, 0, a) || a.commits.size() != K - 1) { fprintf(stderr, "frontier_check: all tied: the replay did not run to K\n"); return false; }
    for (const LqCommit &cm : a.commits)
        if (cm.row != 0) { fprintf(stderr, "frontier_check: all tied: row %d committed, not the first maximum (row 0)\n", cm.row); return false; }
    return true;
}
}  // namespace

int main() {
    static const size_t Ks[] = {2, 3, 15, 16, 17, 32, 33, 256};
    static const Shape shapes[] = {
        {kContinuous, 0, 5}, {kTies, 0, 5}, {kTiny, 0, 10},               // fully evaluated: runs to K, or stops below DELTA
        {kContinuous, 4, 5}, {kTies, 4, 5}, {kTiny, 4, 10},               // a few undecided rows: most stay below the best known one
        {kContinuous, 30, 5}, {kTies, 30, 5},                             // many: the step is blocked
    };
    Rng r{20240607};
    Counts c;
    for (size_t K : Ks)
        for (const Shape &sh : shapes)
            for (int rep = 0; rep < 100; rep++) {
                const int kbase = 1 + (int)r.below((unsigned)std::min<size_t>(12, K));
                const int first_base = (int)r.below(3);
                const std::vector<LqRec> t = make_tree(r, K, kbase, first_base, sh);
                if (!check_tree(t, kbase, first_base, K, c, "random tree")) return 1;
            }
    if (!check_tie_across_blocks(c)) return 1;
    printf("frontier_check: %ld trees agree: %ld ran to K, %ld stopped below DELTA, %ld blocked; the sabotaged step changed %ld results\n",
           c.trees, c.full, c.stopped, c.blocked, c.sabotaged);
    // the cases the trees are made for did occur
    if (c.trees < 3000 || c.full < 100 || c.stopped < 100 || c.blocked < 100 || c.sabotaged < 100) { fprintf(stderr, "frontier_check: a case is missing\n"); return 1; }
    return 0;
}
