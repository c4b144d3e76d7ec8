// split_frontier.h -- the greedy loop of local.c:347-390 over an evaluated candidate tree: plain C++17, no HIP.
// One step (first maximum among the known rows, maximum among the undecided ones, the DELTA stop, the palette-order commit)
// serves both split loops: the replay of the device-driven one (lq_replay) and the host-driven one between its rounds.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace pamd {

struct LqRec {
    double val;                                       // the split's benefit once known, else the bound `ub`
    int left;                                         // left child (right = +1) once the node is in a round, else -1
    int kn;                                           // known: never splits (one member, solver failed) or its split is evaluated
};
struct LqCommit { int row, node, new_row, left; };
struct LqReplay { std::vector<int> result; std::vector<LqCommit> commits; bool stopped_early = false; };

// what a step asks of a node: its split's benefit once known, else the bound; known; the left child (right = +1)
struct FrontierRec { double val; bool known; int left; };

// The frontier in the reference's order (`result`, rows 0 .. count-1) as two flat arrays (benefit if the node's split is known, else
// its bound), in blocks of sixteen rows, each with its first maximum among the known rows and the maximum among the unknown ones: a
// step changes two rows, so it rescans two blocks and the blocks' summaries instead of the whole frontier (254 steps over up to 256
// rows: 50 us of a 1920x1080 call's 1.6 ms before).  `rec(id)` gives a node's FrontierRec.
struct SplitFrontier {
    static constexpr size_t B = 16;
    enum Status { kCommitted, kStopped, kBlocked };
    struct Step { Status status; LqCommit commit; double benefit; };   // commit {row, node, new_row, left} and its benefit: when committed

    std::vector<int> result;
    size_t count = 0;

    // rows 0 .. kbase-1 = the base clusters first_base .. first_base + kbase - 1, room for K rows
    template <class Rec> SplitFrontier(size_t K, int kbase, int first_base, double delta, const Rec &rec)
        : result(std::max(K, (size_t)kbase), -1), count((size_t)kbase), delta_(delta), fval_(blocks(result.size()) * B, 0.0),
          fkn_(fval_.size(), 0), bbv_(blocks(result.size()), 0.0), bmu_(bbv_.size(), -1.0), bbest_(bbv_.size(), -1) {
        for (int j = 0; j < kbase; j++) result[j] = first_base + j;
        reload(rec);
    }
    // the nodes' records changed (a round evaluated them): reload the rows, rescan the blocks
    template <class Rec> void reload(const Rec &rec) {
        for (size_t j = 0; j < count; j++) load(j, rec);
        for (size_t b = 0; b < bbv_.size(); b++) rescan(b);
    }
    // One greedy step, exact whenever every undecided node is provably not the arg-max: first maximum among ALL entries = first
    // maximum among the known ones iff every unknown benefit (<= that node's bound) is strictly below it.  kBlocked: an undecided
    // row could still be the arg-max (reference_benefit() is what it would have to beat).  fault == 2: patolette_amd_debug_fault.
    template <class Rec> Step step(const Rec &rec, int fault) {
        int best = -1; double bv = 0, mu = -1;
        const size_t nbu = blocks(count);
        for (size_t b = 0; b < nbu; b++) {                       // ascending blocks, strict '>': the first maximum of all rows
            if (bbest_[b] >= 0 && (best < 0 || bbv_[b] > bv)) { bv = bbv_[b]; best = bbest_[b]; }
            if (bmu_[b] > mu) mu = bmu_[b];
        }
        ref_ = std::max(best >= 0 ? bv : 0.0, mu);
        if (mu < 0 || (best >= 0 && bv > mu)) {
            if (fault == 2) {                                      // tests only: a WRONG greedy step (the second best known one)
                int second = -1; double sv = -1;
                for (size_t j = 0; j < count; j++) if ((int)j != best && fkn_[j] && fval_[j] > sv) { sv = fval_[j]; second = (int)j; }
                if (second >= 0 && sv >= delta_ && sv < bv) { best = second; bv = sv; }
            }
            if (!(bv >= delta_)) return Step{kStopped, {}, 0.0};               // benefit < DELTA: stop (local.c:365-370)
            const int id = result[best], l = rec(id).left;
            const Step st{kCommitted, LqCommit{best, id, (int)count, l}, bv};
            result[count] = l; result[best] = l + 1;               // local.c:375-376: palette ORDER
            load(count, rec); load((size_t)best, rec);
            count++;
            rescan((size_t)best / B);
            if ((count - 1) / B != (size_t)best / B) rescan((count - 1) / B);
            return st;
        }
        if (ref_ < delta_) return Step{kStopped, {}, 0.0};                     // nothing can reach DELTA
        return Step{kBlocked, {}, 0.0};
    }
    // of the last step: max(first maximum among the known rows, maximum among the undecided ones)
    double reference_benefit() const { return ref_; }
    // the known rows' benefits, in row order
    void known_values(std::vector<double> &out) const {
        out.clear();
        for (size_t j = 0; j < count; j++) if (fkn_[j]) out.push_back(fval_[j]);
    }

private:
    static size_t blocks(size_t rows) { return (rows + B - 1) / B; }
    template <class Rec> void load(size_t j, const Rec &rec) {
        const FrontierRec r = rec(result[j]);
        fval_[j] = r.val; fkn_[j] = r.known ? 1 : 0;
    }
    void rescan(size_t b) {
        int best = -1; double bv = 0, mu = -1;
        const size_t lo = b * B, hi = std::min(count, lo + B);
        for (size_t j = lo; j < hi; j++) {
            if (fkn_[j]) { if (best < 0 || fval_[j] > bv) { bv = fval_[j]; best = (int)j; } }      // first maximum (vector.c:26-46)
            else if (fval_[j] > mu) mu = fval_[j];
        }
        bbest_[b] = best; bbv_[b] = bv; bmu_[b] = mu;
    }
    double delta_, ref_ = 0;
    std::vector<double> fval_;
    std::vector<char> fkn_;
    std::vector<double> bbv_, bmu_;
    std::vector<int> bbest_;
};

// The greedy loop over the evaluated candidate tree of the device-driven split loop (rec: per node the split's benefit once known,
// else the bound; the left child; known).  Exactly the host-driven loop's steps, except that nothing is left to evaluate: false if
// a step is blocked by an undecided node all the same (the device's selection rule forbids it; out.result keeps its K rows then).
inline bool lq_replay(const LqRec *rec, int kbase, int first_base, size_t K, double delta, int fault, LqReplay &out) {
    const auto get = [rec](int id) { return FrontierRec{rec[id].val, rec[id].kn != 0, rec[id].left}; };
    SplitFrontier f(K, kbase, first_base, delta, get);
    bool ok = true;
    while (ok && f.count < K) {
        const SplitFrontier::Step st = f.step(get, fault);
        if (st.status == SplitFrontier::kCommitted) { out.commits.push_back(st.commit); continue; }
        if (st.status == SplitFrontier::kStopped) { out.stopped_early = true; break; }
        ok = false;
    }
    if (ok) f.result.resize(f.count);
    out.result.swap(f.result);
    return ok;
}

// the same loop over the whole frontier at every step (the reference's shape), on no shared code: what PAMD_LQ_REPLAY_CHECK=1 and the
// failure diagnostic hold lq_replay to
inline bool lq_replay_plain(const LqRec *rec, int kbase, int first_base, size_t K, double delta, int fault, LqReplay &out) {
    std::vector<int> &result = out.result;
    result.assign(K, -1);
    for (int j = 0; j < kbase; j++) result[j] = first_base + j;
    size_t count = (size_t)kbase;
    std::vector<double> fval(K, 0.0);
    std::vector<char> fkn(K, 0);
    for (size_t j = 0; j < count; j++) { fval[j] = rec[result[j]].val; fkn[j] = (char)rec[result[j]].kn; }
    while (count < K) {
        int best = -1; double bv = 0, mu = -1;
        for (size_t j = 0; j < count; j++) {
            if (fkn[j]) { if (best < 0 || fval[j] > bv) { bv = fval[j]; best = (int)j; } }      // first maximum (vector.c:26-46)
            else if (fval[j] > mu) mu = fval[j];
        }
        if (mu < 0 || (best >= 0 && bv > mu)) {
            if (fault == 2) {                                      // tests only: a WRONG greedy step (the second best known one)
                int second = -1; double sv = -1;
                for (size_t j = 0; j < count; j++) if ((int)j != best && fkn[j] && fval[j] > sv) { sv = fval[j]; second = (int)j; }
                if (second >= 0 && sv >= delta && sv < bv) { best = second; bv = sv; }
            }
            if (!(bv >= delta)) { out.stopped_early = true; break; }          // benefit < DELTA: stop (local.c:365-370)
            const int id = result[best], l = rec[id].left;
            out.commits.push_back(LqCommit{best, id, (int)count, l});
            result[count] = l; result[best] = l + 1;               // local.c:375-376: palette ORDER
            fval[count] = rec[l].val; fkn[count] = (char)rec[l].kn;
            fval[best] = rec[l + 1].val; fkn[best] = (char)rec[l + 1].kn;
            count++;
            continue;
        }
        if (std::max(best >= 0 ? bv : 0.0, mu) < delta) { out.stopped_early = true; break; }
        return false;
    }
    result.resize(count);
    return true;
}

}  // namespace pamd
