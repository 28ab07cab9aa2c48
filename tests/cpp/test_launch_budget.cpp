// test_launch_budget.cpp — the adaptive launch budget of the north-star solve (dynfu_amd/csrc/launch_budget.hpp) on the
// CPU: no HIP, no library.  `Plan` below is the host side of dfa_solver6_solve around the budget (capi_solver6.cpp) with a model
// of the device and of the pinned mirror: a solve's counts reach its mirror slot when the host waits for its completion
// event and no sooner (`late`: the host as far ahead as the ring allows) or at once (`!late`).  The model keeps, per slot,
// the solve it was last zeroed for, and fails when a slot is written or read for another solve than that.
#include <algorithm>
#include <vector>

#include "../../dynfu_amd/csrc/launch_budget.hpp"
#include "minitest.hpp"

using namespace dfa;
typedef unsigned long long u64;
typedef std::vector<int> Counts;  // PCG iterations per Gauss-Newton iteration of one solve, as the device reports them

static const BudgetKey KEY{2048, 262144, 2, 3, 64, 1e-3f, 0.1f, 0.5f, 0.9f, 1e-3f};
static const int CAP = 64;

struct Plan {
    LaunchBudget budget;
    bool late;
    int mirror[S6_RING][S6_HIST] = {};
    long long owner[S6_RING]     = {-1, -1, -1, -1};  // the solve a slot was last zeroed for
    std::vector<Counts> counts;                       // by solve
    std::vector<bool> complete;
    std::vector<std::vector<u64>> folds;              // by solve: what it folded, in order
    u64 waits = 0;
    explicit Plan(bool late_ = true) : late(late_) {}

    void finish(u64 f) {  // the device ends solve f: its counts are in the mirror
        if (complete[f]) return;
        ASSERT_EQ(owner[f % S6_RING], (long long)f);
        for (size_t gi = 0; gi < std::min<size_t>(counts[f].size(), S6_HIST); ++gi) mirror[f % S6_RING][gi] = counts[f][gi];
        complete[f] = true;
    }
    void wait(u64 f) { ++waits, finish(f); }  // hipEventSynchronize(done_ev[f % S6_RING])

    // one solve as capi_solver6.cpp drives it -> the launches of each of its PCGs
    Counts solve(bool adaptive, const BudgetKey& key, const Counts& device_counts, int cap = CAP) {
        const LaunchBudget::Start b = budget.start(adaptive, key);
        ASSERT_EQ(b.n, (u64)counts.size());
        ASSERT_EQ(b.slot, (int)(b.n % S6_RING));
        folds.push_back({});
        for (u64 f = b.fold_from; f < b.fold_to; ++f) {
            wait(f);
            ASSERT_EQ(owner[f % S6_RING], (long long)f);  // not re-zeroed for a later solve
            ASSERT_EQ(budget.folded, f);
            budget.fold(mirror[f % S6_RING]);
            folds.back().push_back(f);
        }
        if (b.reset) budget.forget(b.n);
        ASSERT_EQ(b.slot_reused, b.n >= (u64)S6_RING);
        if (b.slot_reused) wait(b.n - S6_RING);
        std::fill(mirror[b.slot], mirror[b.slot] + S6_HIST, 0);
        owner[b.slot]          = (long long)b.n;
        budget.slot_gn[b.slot] = (int)device_counts.size();
        Counts launches;
        for (int gi = 0; gi < (int)device_counts.size(); ++gi) launches.push_back(budget.launches(gi, cap));
        counts.push_back(device_counts), complete.push_back(false);
        if (!late) finish(b.n);
        return launches;
    }
};

// the statement of tests/test_gpu_solve6.py::test_adaptive_launch_budget: the budget of solve i from solves first .. i - 2
static int want_launches(const std::vector<Counts>& seen, size_t first, size_t i, int gi, int cap) {
    int pred = 0;
    for (size_t j = first; j + 2 <= i; ++j) pred = std::max(seen[j][gi], pred - 1);
    return pred > 0 ? std::min(cap, pred + std::max(2, pred / 4)) : cap;
}

TEST(LaunchBudget, FirstTwoSolvesGetTheCap) {
    Plan p;
    for (int i = 0; i < 2; ++i) ASSERT_TRUE(p.solve(true, KEY, Counts(40, 5)) == Counts(40, CAP));
    const Counts third = p.solve(true, KEY, Counts(40, 5));
    for (int gi = 0; gi < 40; ++gi) ASSERT_EQ(third[gi], gi < S6_HIST ? 7 : CAP);  // beyond the history: always the cap
    ASSERT_EQ(p.budget.launches(S6_HIST, CAP), CAP);
}

TEST(LaunchBudget, RunningMaximumPlusAQuarterAtLeastTwo) {
    // gi 0 rises by more than a quarter per solve and then falls back, gi 1 falls to 1, gi 2 would exceed the cap
    std::vector<Counts> seen = {{8, 20, 60}, {8, 15, 60}, {12, 9, 61}, {20, 4, 64}, {30, 1, 64}, {30, 1, 50}};
    seen.resize(30, Counts{9, 1, 50});  // (a prediction comes down by one per solve: 20 needs as many solves to reach 1)
    for (int late = 0; late < 2; ++late) {  // the budgets do not depend on how far the device has got
        Plan p(late != 0);
        for (size_t i = 0; i < seen.size(); ++i) {
            const Counts got = p.solve(true, KEY, seen[i]);
            for (int gi = 0; gi < 3; ++gi) ASSERT_EQ(got[gi], want_launches(seen, 0, i, gi, CAP));
            // the fold list: exactly the not-yet-folded solves <= n - 2, in ascending order (here: one per solve)
            ASSERT_TRUE(p.folds[i] == (i >= 2 ? std::vector<u64>{i - 2} : std::vector<u64>{}));
        }
        ASSERT_EQ(p.budget.pred[1], 1);
        ASSERT_EQ(p.budget.launches(1, CAP), 3);
        ASSERT_EQ(p.budget.launches(1, 2), 2);
    }
}

TEST(LaunchBudget, CutSkippedAndSilentSlots) {
    Plan p;
    auto pred_after = [&](const Counts& c) {  // c folded: two solves later
        p.solve(true, KEY, c), p.solve(true, KEY, Counts(c.size(), 0)), p.solve(true, KEY, Counts(c.size(), 0));
        return Counts(p.budget.pred, p.budget.pred + c.size());
    };
    // (between the cases two solves of zeros are folded: seen == 0 leaves pred alone)
    ASSERT_TRUE(pred_after({10, 10, 10, 0}) == (Counts{10, 10, 10, 0}));
    // a cut PCG (seen < 0) raises pred to at least -2 * seen and never lowers it
    ASSERT_TRUE(pred_after({-7, -5, -4, -3}) == (Counts{14, 10, 10, 6}));
    // S6_MIRROR_SKIPPED lowers by one, not below 1, and an unknown slot becomes 1 (never back to 0 = the full cap)
    const Counts skipped(4, S6_MIRROR_SKIPPED);
    ASSERT_TRUE(pred_after(skipped) == (Counts{13, 9, 9, 5}));
    Plan q;
    q.solve(true, KEY, {2, 0});
    for (int i = 0; i < 5; ++i) q.solve(true, KEY, Counts(2, S6_MIRROR_SKIPPED));
    ASSERT_TRUE(Counts(q.budget.pred, q.budget.pred + 2) == (Counts{1, 1}));  // {2, 0} and three skipped solves folded
    ASSERT_EQ(q.budget.launches(1, CAP), 3);
    for (int gi = 2; gi < S6_HIST; ++gi) ASSERT_EQ(q.budget.pred[gi], 0);  // only the slots a solve enqueued are folded
}

TEST(LaunchBudget, ResetTest) {
    auto with = [](int D, int N) {
        BudgetKey k = KEY;
        k.D = D, k.N = N;
        return k;
    };
    ASSERT_TRUE(!budget_key_resets(KEY, KEY));
    // exactly an eighth (of the larger) does not reset, one more does — either direction, D and N alike
    ASSERT_TRUE(!budget_key_resets(with(1024, KEY.N), with(896, KEY.N)) && !budget_key_resets(with(896, KEY.N), with(1024, KEY.N)));
    ASSERT_TRUE(budget_key_resets(with(1024, KEY.N), with(895, KEY.N)) && budget_key_resets(with(895, KEY.N), with(1024, KEY.N)));
    ASSERT_TRUE(!budget_key_resets(with(KEY.D, 80000), with(KEY.D, 70000)) && budget_key_resets(with(KEY.D, 80000), with(KEY.D, 69999)));
    // any change of iteration counts or tolerances resets
    for (int field = 0; field < 8; ++field) {
        BudgetKey k = KEY;
        int* ints[]     = {&k.num_iter, &k.gn_iter, &k.linear_iter};
        float* floats[] = {&k.tol, &k.tol_first, &k.tol_decay, &k.tol_adapt, &k.gn_tol};
        if (field < 3) *ints[field] += 1;
        else *floats[field - 3] *= 1.0000002f;
        ASSERT_TRUE(budget_key_resets(k, KEY) && budget_key_resets(KEY, k));
    }
}

TEST(LaunchBudget, BehindAResetTwoSolvesGetTheCapAndTheOldProblemIsForgotten) {
    for (int late = 0; late < 2; ++late) {
        Plan p(late != 0);
        std::vector<Counts> seen;
        for (int i = 0; i < 5; ++i) seen.push_back({40 + i, 50}), p.solve(true, KEY, seen.back());
        BudgetKey other = KEY;
        other.D = KEY.D / 2;
        for (int i = 5; i < 11; ++i) {
            seen.push_back({3, 6});
            const Counts got = p.solve(true, other, seen.back());
            // solves 3 and 4 — the two before the reset — never reach a budget: it is a function of solves 5 .. i - 2
            for (int gi = 0; gi < 2; ++gi) ASSERT_EQ(got[gi], want_launches(seen, 5, i, gi, CAP));
            if (i < 7) ASSERT_TRUE(got == (Counts{CAP, CAP}));
            if (i > 5) ASSERT_TRUE(std::find(p.folds[i].begin(), p.folds[i].end(), 4ull) == p.folds[i].end());
        }
        ASSERT_TRUE(p.folds[7] == std::vector<u64>{5});
    }
}

TEST(LaunchBudget, ASolveWithoutABudgetClearsTheHistory) {
    // Solve n without adaptive_launch gets the cap, clears the history and drops the folds still outstanding; the solves
    // behind it start again from folded = n - 1, as if every solve before that were in the history.  (So the counts of
    // solves n - 1 and n themselves — the mirror is written with or without a budget — are folded by solves n + 1 and
    // n + 2 in the ordinary way; nothing earlier ever is.  This is what the code has always done, pinned here as it is.)
    Plan p;
    std::vector<Counts> seen;
    for (int i = 0; i < 4; ++i) seen.push_back({30}), p.solve(true, KEY, seen.back());
    ASSERT_EQ(p.budget.pred[0], 30);
    seen.push_back({5});
    ASSERT_TRUE(p.solve(false, KEY, seen.back()) == Counts{CAP});  // n = 4
    ASSERT_TRUE(p.folds[4].empty() && p.budget.pred[0] == 0 && p.budget.folded == 3);
    for (int i = 5; i < 9; ++i) {
        seen.push_back({5});
        const Counts got = p.solve(true, KEY, seen.back());
        ASSERT_EQ(got[0], want_launches(seen, 3, i, 0, CAP));
        ASSERT_TRUE(p.folds[i] == std::vector<u64>{(u64)i - 2});  // 3, 4, 5, 6: never 2
    }
    // several in a row: the ones in between are never folded
    for (int i = 9; i < 12; ++i) seen.push_back({50}), ASSERT_TRUE(p.solve(false, KEY, seen.back()) == Counts{CAP});
    seen.push_back({5});
    p.solve(true, KEY, seen.back());
    ASSERT_TRUE(p.folds[12] == std::vector<u64>{10});
    // the very first solve of a plan without a budget
    Plan q;
    ASSERT_TRUE(q.solve(false, KEY, {9}) == Counts{CAP} && q.budget.folded == 0);
    ASSERT_TRUE(q.solve(false, KEY, {9}) == Counts{CAP} && q.budget.folded == 0);
    // (the first solve with a budget meets no key to compare with: a reset, and two solves at the cap behind it)
    ASSERT_TRUE(q.solve(true, KEY, {9}) == Counts{CAP} && q.folds[2] == std::vector<u64>{0} && q.budget.folded == 2);
    ASSERT_TRUE(q.solve(true, KEY, {9}) == Counts{CAP} && q.solve(true, KEY, {9}) == Counts{11});
}

TEST(LaunchBudget, RingWithTheHostThreeSolvesAhead) {
    // Solves without a budget fold nothing, so nothing makes the host wait but the reuse of a slot: the device may be
    // S6_RING - 1 = 3 solves behind.  Adaptive solves behind them: every fold list is exactly the not-yet-folded solves
    // <= n - 2 in ascending order, and Plan::solve has checked that each slot still belonged to the solve folded from it.
    Plan p;
    std::vector<Counts> seen;
    BudgetKey key = KEY;
    auto run = [&](bool adaptive, int it) { seen.push_back({it}), p.solve(adaptive, key, seen.back()); };
    run(true, 20);
    for (int i = 1; i < 7; ++i) run(false, 20 + i);
    ASSERT_EQ(p.waits, 3ull);  // solves 0, 1, 2, each when its slot was taken again
    ASSERT_TRUE(p.complete[2] && !p.complete[3] && !p.complete[4] && !p.complete[5] && !p.complete[6]);
    u64 folded = p.budget.folded;
    ASSERT_EQ(folded, 5ull);
    for (int i = 7; i < 20; ++i) {
        run(true, 20 + i);
        std::vector<u64> want;
        for (; folded + 2 <= (u64)i; ++folded) want.push_back(folded);
        ASSERT_TRUE(p.folds[i] == want);
        ASSERT_EQ(p.budget.folded, folded);
        ASSERT_EQ(p.budget.pred[0], 20 + i - 2);
    }
    // a reset leaves a backlog of one (solve n - 1 is skipped): the lists stay in order and within the ring
    run(true, 7);
    key.gn_iter += 1;
    run(true, 7);
    ASSERT_TRUE(p.folds[21] == std::vector<u64>{19} && p.budget.folded == 21);
    for (int i = 22; i < 30; ++i) {
        run(true, 7);
        ASSERT_TRUE(p.folds[i] == (i >= 23 ? std::vector<u64>{(u64)i - 2} : std::vector<u64>{}));
    }
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
