// launch_budget.hpp — the adaptive launch budget of the north-star solve (dfa_solve6_params.adaptive_launch; DESIGN.md
// §4.5) as host-only code: no HIP header, plain g++ compiles it (tests/cpp/test_launch_budget.cpp drives it on the CPU).
//
// The device writes the PCG iterations of every Gauss-Newton iteration of solve n into slot n % S6_RING of a pinned
// mirror; the budget of solve n is a function of the solves up to n - 2 ONLY, folded into the history in order behind
// their completion events — never of how far the device happens to have got: the same sequence of solves gets the same
// budgets in every run.
//
// This header decides; capi_solver6.cpp keeps every HIP call.  Per solve:
//     b = start(adaptive, key)
//     for f in [b.fold_from, b.fold_to):  wait for the completion event of slot f % S6_RING;  fold(its mirror slot)
//     if (b.reset) forget(b.n)
//     if (b.slot_reused) wait for the completion event of slot b.slot;  zero that mirror slot;  slot_gn[b.slot] = ...
//     launches(gi, cap) for every PCG;  record the completion event of slot b.slot behind the last launch
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>

#pragma GCC visibility push(hidden)  // internal to the library: nothing here joins its exported symbols
namespace dfa {

constexpr int S6_HIST = 32;  // = DFA_SOLVE6_HIST of include/dynfu_amd.h
constexpr int S6_MIRROR_SKIPPED = -(1 << 30);  // launch-budget mirror: the Gauss-Newton iteration ran no PCG (its outer iteration had ended)
constexpr int S6_RING = 4;  // mirror slots: the host may run S6_RING - 1 solves ahead of the device without waiting

// what a prediction is valid for: another problem, or other stopping rules, and what the last one needed says nothing
struct BudgetKey {
    int D, N, num_iter, gn_iter, linear_iter;
    float tol, tol_first, tol_decay, tol_adapt, gn_tol;
};

inline bool budget_key_resets(const BudgetKey& key, const BudgetKey& old) {
    auto far = [](int a, int b) { return std::abs(a - b) * 8 > std::max(a, b); };  // changed by more than an eighth
    return far(key.D, old.D) || far(key.N, old.N) || key.num_iter != old.num_iter || key.gn_iter != old.gn_iter ||
           key.linear_iter != old.linear_iter || key.tol != old.tol || key.tol_first != old.tol_first ||
           key.tol_decay != old.tol_decay || key.tol_adapt != old.tol_adapt || key.gn_tol != old.gn_tol;
}

struct LaunchBudget {
    int pred[S6_HIST] = {};  // iterations per Gauss-Newton iteration: raised at once, lowered by one per solve; 0 = unknown
    BudgetKey key = {};
    unsigned long long solve_seq = 0, folded = 0;  // solves started; solves whose counts are in the history
    int slot_gn[S6_RING] = {};                     // Gauss-Newton iterations solve n enqueued, by n % S6_RING

    struct Start {
        unsigned long long n;                   // this solve
        int slot;                               // its mirror slot
        unsigned long long fold_from, fold_to;  // the earlier solves to fold now, in order: [fold_from, fold_to)
        bool reset;                             // behind the folds: forget(n)
        bool slot_reused;                       // the slot's previous owner, solve n - S6_RING, must have finished writing it
    };

    // solve n begins, with a budget (adaptive) or with the caller's cap for every PCG
    Start start(bool adaptive, const BudgetKey& k) {
        const unsigned long long n = solve_seq++;
        Start b{n, (int)(n % S6_RING), folded, folded, false, n >= (unsigned long long)S6_RING};
        if (adaptive) {
            b.reset = budget_key_resets(k, key);
            key     = k;
            if (n >= 2) b.fold_to = std::max(folded, n - 1);  // the solves up to n - 2
        } else {
            folded = n + 1 >= 2 ? n - 1 : 0;  // nothing to fold later from solves without a budget
            std::memset(pred, 0, sizeof(pred));
            b.fold_from = b.fold_to = folded;
        }
        return b;
    }

    // the counts of solve `folded` (complete: its mirror slot is final) enter the history
    void fold(const int* counts) {
        const int gn = std::min(slot_gn[folded % S6_RING], S6_HIST);
        for (int gi = 0; gi < gn; ++gi) {
            const int seen = counts[gi];
            int& p         = pred[gi];
            // (an iteration behind the end of its outer iteration ran no PCG: its budget decays like one that needed
            // little — the launches enqueued for it are no-ops every time it is skipped again — but stays known)
            if (seen == S6_MIRROR_SKIPPED) p = p > 1 ? p - 1 : 1;  // (never back to 0 = unknown = the full cap)
            else if (seen > 0) p = std::max(seen, p - 1);
            else if (seen < 0) p = std::max(p, -2 * seen);  // cut short: twice as many
        }
        ++folded;
    }

    // another problem (or other stopping rules): what the previous one needed says nothing
    void forget(unsigned long long n) {
        std::memset(pred, 0, sizeof(pred));
        folded = n;  // (solves n - 2, n - 1 of the old problem are never folded)
    }

    // Launches of the PCG of Gauss-Newton iteration gi: the caller's cap, or what this iteration needed in the plan's
    // earlier solves (a maximum that decays by one per solve) plus a quarter, at least two.  (Measured at C2 / C3 over
    // 30-frame sequences: consecutive frames move a count by up to 2 where it is small and by up to a quarter where it is
    // 30-40; one launch of slack instead of two cut 1-2 PCGs short in a fifth of the frames.)
    // (VERDICT r05 item 7 — one launch of slack where a slot's count had repeated in two solves running, one launch for a
    // slot skipped twice running — was built and measured in round 6: 58 launches for 41 iterations instead of 60 for 36
    // at C2, 83 for 53 instead of 92 for 47 at C3, and the frames/s inside the run-to-run spread (863.6 against 860,
    // 331 against 343 over the whole period): a launch that returns at entry costs 3.5 us, a dozen of them 3 % of a
    // C2 frame.  Not kept.)
    int launches(int gi, int cap) const {
        if (gi >= S6_HIST || pred[gi] <= 0) return cap;  // (a solve without a budget has cleared the history)
        return std::min(cap, pred[gi] + std::max(2, pred[gi] / 4));
    }
};

}  // namespace dfa
#pragma GCC visibility pop
