// bz_options.h -- the search options (BZ_OPT_*, include/bz_abi.h) and THE table of the pairs that do not run together (DESIGN.md 5,
// "The search mode").  Plain C++, no HIP: the setters and the *_bytes / *_check entry points refuse from it at run time
// (option_refusal in bz_mcts.hip, through refuse_first_conflict), Mode<M> refuses the same pairs at compile time (mode_served), and
// bz_option_conflict / bz_option_name let a test read it without a GPU.  betazero_amd/engine.py keeps the same pairs under its keyword names (SEARCH_OPTION_CONFLICTS);
// tests/test_option_conflicts_cpu.py holds the two equal.
#pragma once
#include <stdint.h>

#include "../../include/bz_abi.h"

namespace bz {
void set_error(const char* fmt, ...);  // (bz_common.h)

// ---- The search mode: which rules the walk (dev_select), the tree step around it (tree_step_body) and the move (play_body, which
// says what each bit does to the move) run under.  One bit per rule, one compile-time mask M per kernel; the host derives the same
// mask from the engine (engine_mode) and switches over it.  With no bit set the code is k_tree_step's / k_play's exactly.
enum : unsigned {
    // kModeLeaf (k_leaf_step): K > 1 walks per game per step.  In the walk, a non-terminal child without edges was
    // created by an earlier walk of this step and ends the walk as LEAF_COLLIDE; the evaluation cache is not consulted.
    kModeLeaf = 1u << 0,
    // kModeGumbel (k_gumbel_step): the root's edge is chosen by gumbel_root_pick instead of PUCT (every deeper
    // level is PUCT), and v_root is stored with the root's expansion.
    kModeGumbel = 1u << 1,
    // kModeCap (k_cap_step): the walk runs only while sim_idx is below the slot's budget.
    kModeCap = 1u << 2,
    // kModeForced (k_forced_step / k_forced_cap_step): at the root an edge with 0 < N < fsqrt(fk P sumN) scores +inf
    // (fk = 0: this slot does not force -- under kModeCap the full searches only force); every deeper level is PUCT.
    kModeForced = 1u << 3,
    // kModeFpu (k_fpu_*_step): at every level an edge with N == 0 takes q = the node's own value minus a reduction
    // that grows with the prior mass of the node's visited edges, instead of 0.  The mass needs all of the node's edges before any
    // is scored: its <= kCH chunks are loaded together into registers (still ONE dependent load per level), summed as integers
    // across the group, then scored from the registers.  The root's running value sum Wr is loaded with the per-game words,
    // advanced by what this step's backup adds to the path's root edge and stored beside it.  sim_idx is the number of simulations
    // backed up once this step's backup is done (an expand-only step gets it from the host too): the backup of simulation 0 starts
    // Wr from 0, so no search needs a reset.
    kModeFpu = 1u << 4,
    // kModeGfull (k_gfull_step; with kModeGumbel): every level below the root takes the edge whose visit share lags
    // the node's improved policy softmax(logf(P~) + sigma(completed Q)) the most, in place of PUCT.  Like kModeFpu the node's <= kCH
    // edge chunks are loaded together into registers, and the node's own value v_X (this game's row of the interior buffer) is
    // loaded beside its position: still ONE dependent load per level.  Per-edge terms are computed one edge per lane; max / min are
    // group reductions; the three sums run in ascending edge order (group_seq_sum), so the bits are those of gi_pick_serial.  Every
    // expanded node's value is stored in the interior buffer with its expansion, on the EVAL and on the COPY path.
    kModeGfull = 1u << 5,
    // kModeSolve (k_solve_step / k_solve_cap_step; the plain PUCT branch of the walk only): a decided edge (terminal
    // or proven) with c = -1 scores +inf, with c = +1 -inf, with c = 0 takes q = 0; when every edge scores -inf the walk takes edge
    // 0; a walk that takes a decided edge ends there with the edge's value, as at a terminal edge.  The proof pass runs behind the
    // backup of a terminal or proven leaf; the backup of an evaluated or copied leaf stays the pure-store path it is.
    kModeSolve = 1u << 6,
    // kModeStop (k_stop_step / k_fpu_stop_step): behind the backup of the step of simulation s, a slot whose move is
    // decided (early_stop_decided over the root's visits, s done, sims - s to go) and not sampled (moves made >= temp_moves)
    // records stop_at = s, selects nothing and is left LEAF_NONE: idle from then on, like a slot at its playout-cap budget.  The
    // root's first kGW edges are the ones patched in registers, the others are loaded behind the group fence; the leader and the
    // "can still catch up" flag are two group reductions, skipped per game while early_stop_possible says the rule cannot fire.
    kModeStop = 1u << 7,
    // kModePace (k_pace_step, DESIGN.md 3.11 "The replay seed"): a slot whose tree k_replay_seed filled with the first `seeded`
    // simulations of its search walks only in the launches csrc/bz_pace.h gives its remaining ones, as simulation seeded + (walks
    // made so far) instead of the launch index, and is left LEAF_NONE in the others; its root came expanded, so the root's net row
    // is counted and nothing is written for it.  A slot with seeded = 0 walks in every launch: k_tree_step's search.
    kModePace = 1u << 8,
};

// ---- One row per option, indexed by its BZ_OPT_* id: the phrase the messages use (a phrase that ends in "s" is a plural: "do
// not combine"), how a caller switches it on, and its bit of the search mode (0: it changes no step kernel).  Whether an option
// is on is read from the engine or its config in one place, option_on (bz_mcts.hip, next to struct bz_engine).
struct OptionRow { const char* phrase; const char* how; unsigned mode; };
constexpr OptionRow kOptions[BZ_OPT_COUNT] = {
    /* BZ_OPT_REUSE_SUBTREE   */ {"subtree reuse", "BZ_ENGINE_REUSE_SUBTREE", 0u},
    /* BZ_OPT_LEAVES          */ {"leaves_per_step > 1", "BZ_ENGINE_LEAVES_*", kModeLeaf},
    /* BZ_OPT_DIRICHLET       */ {"Dirichlet noise", "dirichlet_eps > 0", 0u},
    /* BZ_OPT_GUMBEL          */ {"Gumbel root search", "bz_engine_set_gumbel", kModeGumbel},
    /* BZ_OPT_GUMBEL_INTERIOR */ {"the Gumbel interior rule", "bz_engine_set_gumbel_interior", kModeGfull},
    /* BZ_OPT_PLAYOUT_CAP     */ {"playout cap randomisation", "bz_engine_set_playout_cap", kModeCap},
    /* BZ_OPT_FORCED_PLAYOUTS */ {"forced playouts", "bz_engine_set_forced_playouts", kModeForced},
    /* BZ_OPT_FPU             */ {"first-play urgency reduction", "bz_engine_set_fpu", kModeFpu},
    /* BZ_OPT_SOLVER          */ {"the solver", "bz_engine_set_solver", kModeSolve},
    /* BZ_OPT_EARLY_STOP      */ {"early stop", "bz_engine_set_early_stop", kModeStop},
    /* BZ_OPT_ROOT_STORE      */ {"the root store", "bz_engine_set_root_store", 0u},
    /* BZ_OPT_SURPRISE        */ {"policy surprise weighting", "bz_engine_set_surprise", 0u},
    /* BZ_OPT_SEARCH_VALUE    */ {"search-value targets", "bz_engine_set_search_value", 0u},
    /* BZ_OPT_OWNERSHIP       */ {"ownership targets", "bz_engine_set_ownership", 0u},
    /* BZ_OPT_RESIGN          */ {"resignation", "bz_engine_set_resign", 0u},
};

// ---- The pairs that do not run together, each once and in either order; the reason, where there is one, ends the message.  The
// config-carried options come first, so a refusal names them before an option another setter switched on.  ("The Gumbel interior
// rule needs Gumbel root search" is a requirement, not a conflict: bz_engine_set_gumbel_interior and Mode state it themselves.)
struct OptionConflict { int a, b; const char* reason; };
constexpr OptionConflict kConflicts[] = {
    {BZ_OPT_REUSE_SUBTREE, BZ_OPT_GUMBEL, nullptr},
    {BZ_OPT_REUSE_SUBTREE, BZ_OPT_PLAYOUT_CAP, nullptr},
    {BZ_OPT_REUSE_SUBTREE, BZ_OPT_FORCED_PLAYOUTS, nullptr},
    {BZ_OPT_REUSE_SUBTREE, BZ_OPT_FPU, nullptr},
    {BZ_OPT_REUSE_SUBTREE, BZ_OPT_SOLVER, nullptr},
    {BZ_OPT_REUSE_SUBTREE, BZ_OPT_EARLY_STOP, nullptr},
    {BZ_OPT_LEAVES, BZ_OPT_GUMBEL, nullptr},
    {BZ_OPT_LEAVES, BZ_OPT_PLAYOUT_CAP, nullptr},
    {BZ_OPT_LEAVES, BZ_OPT_FORCED_PLAYOUTS, nullptr},
    {BZ_OPT_LEAVES, BZ_OPT_FPU, nullptr},
    {BZ_OPT_LEAVES, BZ_OPT_SOLVER, "concurrent walks race on proofs"},
    {BZ_OPT_LEAVES, BZ_OPT_EARLY_STOP, nullptr},
    {BZ_OPT_DIRICHLET, BZ_OPT_GUMBEL, nullptr},
    {BZ_OPT_GUMBEL, BZ_OPT_PLAYOUT_CAP, nullptr},
    {BZ_OPT_GUMBEL, BZ_OPT_FORCED_PLAYOUTS, nullptr},
    {BZ_OPT_GUMBEL, BZ_OPT_FPU, nullptr},
    {BZ_OPT_GUMBEL, BZ_OPT_SOLVER, nullptr},
    {BZ_OPT_GUMBEL, BZ_OPT_EARLY_STOP, "sequential halving is its own schedule"},
    {BZ_OPT_SOLVER, BZ_OPT_FORCED_PLAYOUTS, "both score +inf"},
    {BZ_OPT_SOLVER, BZ_OPT_FPU, nullptr},
    {BZ_OPT_SOLVER, BZ_OPT_EARLY_STOP, nullptr},
    {BZ_OPT_EARLY_STOP, BZ_OPT_PLAYOUT_CAP, nullptr},
    {BZ_OPT_EARLY_STOP, BZ_OPT_FORCED_PLAYOUTS, nullptr},
    {BZ_OPT_EARLY_STOP, BZ_OPT_ROOT_STORE, "a shortened tree must not seed a later search"},
    {BZ_OPT_EARLY_STOP, BZ_OPT_SURPRISE, "its targets come from complete searches"},
    {BZ_OPT_EARLY_STOP, BZ_OPT_SEARCH_VALUE, "its targets come from complete searches"},
    {BZ_OPT_EARLY_STOP, BZ_OPT_OWNERSHIP, "its targets come from complete searches"},
    {BZ_OPT_EARLY_STOP, BZ_OPT_RESIGN, "its records come from complete searches"},
    {BZ_OPT_OWNERSHIP, BZ_OPT_RESIGN, "a resigned game has no final board"},
};

constexpr bool option_id_ok(int opt) { return opt >= 0 && opt < BZ_OPT_COUNT; }
constexpr bool option_conflict(int a, int b) {
    for (const OptionConflict& c : kConflicts)
        if ((c.a == a && c.b == b) || (c.a == b && c.b == a)) return true;
    return false;
}
// whether some kernel may serve the search mode M as far as this table goes: no two of its bits belong to a refused pair
constexpr bool mode_served(unsigned M) {
    for (const OptionConflict& c : kConflicts)
        if ((M & kOptions[c.a].mode) && (M & kOptions[c.b].mode)) return false;  // (an option without a bit: mode 0)
    return true;
}

// The one refusal: walks the table for the first option that is on -- on(id) says so -- and does not run with `opt`, and leaves
// "fn: <opt> does / do not combine with <other> (<how the other is set>)[: reason]" as the error.  True: refused.
template <class On>
bool refuse_first_conflict(const char* fn, int opt, On&& on) {
    for (const OptionConflict& c : kConflicts) {
        if (c.a != opt && c.b != opt) continue;
        const int other = c.a == opt ? c.b : c.a;
        if (!on(other)) continue;
        const char* p = kOptions[opt].phrase;
        int n = 0;
        while (p[n]) ++n;
        set_error("%s: %s %s not combine with %s (%s)%s%s", fn, p, p[n - 1] == 's' ? "do" : "does", kOptions[other].phrase,
                  kOptions[other].how, c.reason ? ": " : "", c.reason ? c.reason : "");
        return true;
    }
    return false;
}

}  // namespace bz
