// bz_mcts.hip -- batched MCTS self-play engine for gfx950.
//
// G::GW lanes serve one game (Reversi 16, TTT 4).  Per game the tree is a bump-allocated AoS
// pair in HBM:
//   Node 32 B {own, opp, legal, edge0, info}     nodes[g][sims+2]
//   Edge 16 B {w0, W, P, w3}                     edges[g][(sims+2)*MAXCH]
//        w0 = N 14 | action 7 | child's edge count 6 | child terminal 1 | child's value 2
//        w3 = child id 13 | child's first edge 19
// One dwordx4 load brings an edge's (N, W, P) AND everything the walk needs to know about the child behind
// it, so a level of the PUCT walk is ONE dependent load (the children's edge block) instead of node-then-
// edges; the node array is read by the walk only for the position of the node it extends (issued beside the
// edge load, off the chain).  The select path is stored game-major as {edge index, w0, W} as seen at
// selection time, so the backup of the next launch is one coalesced load + one 8-byte store per edge (nothing
// else touches a game's tree in between), and the created leaf's legal mask / header go to per-game words, so
// the expansion does not re-read the node.  The words the tree step reads about a game sit in one 64-byte record
// (GameHot); the caller-visible per-game arrays (positions, state, leaf buffers) are SoA across games.  A simulation is two
// launches: k_tree_step ([expand + backup of the previous leaf] + [select of the next one]) and the evaluator;
// leaves that need the net are packed through a double-buffered device-side counter.
// Synthetic evaluators run the whole search in one launch (k_search_fused; k_search_fused_ttt for tic-tac-toe at
// sims <= 120: root edges in registers, child header packed into the edge word, path in LDS).  Opt-in: Dirichlet root
// noise (k_root_noise) and subtree reuse (two arenas, dev_reroot) -- DESIGN.md 3.9, 3.10; leaf-parallel search with virtual
// loss (K walks per game per step, k_leaf_step) -- DESIGN.md 3.12.
// First-play urgency reduction in the select rule (k_fpu_step and its cap / forced variants, csrc/bz_fpu.h) -- DESIGN.md 3.20.
// Proven wins, losses and draws (k_solve_step / k_solve_cap_step, the proof pass behind their backup, csrc/bz_solver.h) -- DESIGN.md 3.23.
// The Gumbel interior rule below the root of a Gumbel search (k_gfull_step, csrc/bz_gumbel_interior.h) -- DESIGN.md 3.21.
// Resignation in self-play (k_resign_note in front of the play kernel, k_resign_finish behind it, csrc/bz_resign.h) -- DESIGN.md 3.24.
// Exact early stop of a search whose move is decided (k_stop_step / k_fpu_stop_step, csrc/bz_early_stop.h) -- DESIGN.md 3.25.
// The replay seed: a carried slot's search starts from the played child's old subtree (k_replay_seed behind k_root_begin) and makes
// its remaining walks in its own launches (k_pace_step, csrc/bz_pace.h) -- DESIGN.md 3.11.
//
// Float discipline: compiled with -ffp-contract=off; PUCT / softmax / backup use
// the single-rounding operation order of the oracle (oracle/bz_oracle.c), so
// visit counts, moves and W/P/pi are bit-identical to it.
//
// Reference anchors: turn loop + pass rule reversi_terminal.py:16-38;
// trajectory contract tic_tac_toe.py:13-34; canonical side-to-move states
// generate_training_games.py:12-23.  MCTS itself is build-authored (the
// reference has none).
#include <new>

#include <time.h>

#include "bz_common.h"
#include "bz_math.h"
#include "bz_rules.h"
#include "bz_fpu.h"
#include "bz_solver.h"
#include "bz_early_stop.h"
#include "bz_options.h"
#include "bz_pace.h"
#include "bz_gumbel_interior.h"
#include "bz_surprise.h"
#include "bz_value.h"
#include "bz_ownership.h"
#include "bz_resign.h"

using namespace bz;

namespace {

struct __attribute__((aligned(16))) Node { u64 own, opp, legal; u32 edge0, info; };
struct __attribute__((aligned(16))) Edge { u32 w0; float W; float P; u32 w3; };
static_assert(sizeof(Node) == 32 && sizeof(Edge) == 16, "layout");
// packed edge words (the limits they imply -- nodes per game <= kMaxNodes -- are checked by cfg_ok)
constexpr int kNBits = 14, kActShift = 14, kNchShift = 21, kTermShift = 27, kValShift = 28, kChildBits = 13;
constexpr u32 kNMask = (1u << kNBits) - 1u, kChildMask = (1u << kChildBits) - 1u;
constexpr int kMaxNodes = (1 << kChildBits) - 1;  // also bounds N (<= nodes) and the edge index (19 bits >= 8191 * 34)
__host__ __device__ __forceinline__ u32 e_N(u32 w0) { return w0 & kNMask; }
__host__ __device__ __forceinline__ int e_action(u32 w0) { return (int)((w0 >> kActShift) & 0x7Fu); }
__host__ __device__ __forceinline__ int e_nch(u32 w0) { return (int)((w0 >> kNchShift) & 0x3Fu); }
__host__ __device__ __forceinline__ bool e_term(u32 w0) { return ((w0 >> kTermShift) & 1u) != 0; }
__host__ __device__ __forceinline__ int e_val(u32 w0) { return (int)((w0 >> kValShift) & 3u) - 1; }
//  bit 30 of w0: the edge is PROVEN -- its child is decided with the value in the kValShift bits, for the mover at
// the child like a terminal child's.  Only the proof pass of the solver kernels sets it; every fresh or copied edge has it clear.
constexpr int kProvenShift = 30;
constexpr u32 kProven = 1u << kProvenShift, kDecidedMask = kProven | (1u << kTermShift);
__host__ __device__ __forceinline__ bool e_decided(u32 w0) { return (w0 & kDecidedMask) != 0; }
__host__ __device__ __forceinline__ int e_cval(u32 w0) { return e_decided(w0) ? e_val(w0) : kSolverUndecided; }
__host__ __device__ __forceinline__ u32 e_child(u32 w3) { return w3 & kChildMask; }
__host__ __device__ __forceinline__ u32 e_edge0(u32 w3) { return w3 >> kChildBits; }

constexpr u32 kTerm = 1u << 8;
// leaf_kind: NONE = slot idle; EVAL = the leaf awaits (logits, value); TERMINAL = backup of a terminal value;
// READY = nothing to expand or back up, select at once (a root whose subtree was kept from the previous move);
// COPY = the leaf's position was evaluated earlier in this search (evaluation cache): its priors and value are copied
// from that node instead of going through the evaluator again
// COLLIDE (leaf-parallel search) = the walk stopped at a node an earlier walk of the same step created and
// that is not expanded yet: it takes that node's value and uses no evaluator row
enum { LEAF_NONE = 0, LEAF_EVAL = 1, LEAF_TERMINAL = 2, LEAF_READY = 3, LEAF_COPY = 4, LEAF_COLLIDE = 5 };
enum { CNT_SIMS, CNT_PATH_NODES, CNT_CHILD_SCORED, CNT_EDGES_BACKED, CNT_EXPANDED, CNT_CHILD_WRITTEN,
       CNT_ENV_STEPS, CNT_NET_LEAVES, CNT_CACHE_HITS, CNT_CACHE_HITS_PREV, CNT_N };
// counters[10] (n_collisions, leaf-parallel search only) is not one of the per-wave slots (their layout, and so the
// workspace, stays what it is at K = 1): k_leaf_step adds a wave's collisions straight into it, one atomic per wave that
// has any -- they are rare
constexpr int kCntCollisions = 10;
constexpr int kCntWords = 24;  // u64 words of the counters block: CNT_N work counters, then (diagnostic builds) stamps at 16..23
// NEVAL[2]: packed-leaf counters, double-buffered by simulation parity (the tree step that
// packs into one buffer zeroes the other, so no extra reset launch is needed)
enum { FLAG_ERR = 0, FLAG_FINISHED = 1, FLAG_ACTIVE = 2, FLAG_NEVAL = 4, FLAG_N = 8 };
// ERR_EVAL_NONFINITE: the evaluator handed back a NaN / infinity (a diverged net, an external evaluator's bug): the
// softmax of such a row is NaN, every PUCT comparison with it is false and the search would quietly walk garbage
enum { ERR_EDGE_OVERFLOW = 1, ERR_TERMINAL_ROOT = 2, ERR_EXAMPLE_OVERFLOW = 4, ERR_DEPTH = 8, ERR_EVAL_NONFINITE = 16,
       ERR_REANALYSE_ROW = 32 };  //  a reanalysed row index outside the caller's columns

struct __attribute__((aligned(16))) PathEnt { u32 eidx; u32 w0; float W; u32 pad; };

// the tree step's per-game words in ONE 64-byte line (they were nine arrays: nine cache lines, nine TLB lookups per game at
// the head of every launch, all of them missing the L2 after the net kernel has streamed its weights through it)
struct __attribute__((aligned(64))) GameHot {
    u64 leaf_legal; u32 leaf_node, leaf_info;   // the leaf awaiting expansion / backup: its legal mask, node id, header
    u32 depth, n_nodes, n_edges, leaf_slot;     // its depth; the tree's fill; the evaluator row of the leaf
    u32 root_n, root_base;                      // the root's child count; visits a kept subtree came with (subtree reuse)
    // evaluation cache: this search's generation; a COPY leaf's source node (bit 31: it lives in the PREVIOUS search's arena)
    // and that node's first edge; the generation of the last search this slot took part in and how many nodes the
    // previous search's arena holds for it (0: nothing to carry over)
    // replay seed: the simulations the slot's tree came with in this search (k_replay_seed; kPaceIdle: the slot
    // has no search to run) -- written and read only when the search is paced
    u32 tt_gen, copy_src, copy_e0, last_gen, prev_nodes, seeded;
};
constexpr u32 kSrcPrev = 1u << 31;
static_assert(sizeof(GameHot) == 64, "layout");

// leaf-parallel search (K > 1): what walk j of game g left for the next tree step, at [g][j].
// slot: the evaluator row of an EVAL leaf; v: an expanded leaf's value (what a later walk colliding with its node backs up)
struct __attribute__((aligned(16))) LeafRec { u64 legal; u32 node, info, slot, depth, kind; float v; };
static_assert(sizeof(LeafRec) == 32, "layout");

struct EngineDev {
    int B, ncap, ecap, sims, na, t_max, rounds, temp_moves, openings, maxd, stagger;
    int compact;  // net evaluators: leaves needing evaluation are packed (c_own/c_opp/logits/value by slot)
    int reuse;    // BZ_ENGINE_REUSE_SUBTREE: two tree arenas; nodes/edges = this move's, *_alt = the previous move's
    Node* nodes_alt; Edge* edges_alt; u32* g_reuse;
    float c_puct, dir_alpha, dir_eps;  // dir_eps > 0: Dirichlet noise on the root priors
    u64 seed, id_base, id_stride;
    Node* nodes; Edge* edges;
    u64 *g_own, *g_opp; int8_t* g_to_move; uint8_t* g_state; int32_t *g_moves, *g_nex, *g_round, *g_passes;
    struct GameHot* hot;  // [B]
    PathEnt* path;        // [B][K][maxd], game-major
    int K;                // leaves per step (BZ_ENGINE_LEAVES_*): 1 = k_tree_step, > 1 = k_leaf_step
    LeafRec* lrec;        // [B][K] (K > 1 only)
    uint8_t* leaf_kind; u64 *leaf_own, *leaf_opp, *c_own, *c_opp;
    float *logits, *value;
    u64 *ex_own, *ex_opp; float* ex_pi; int8_t *ex_z, *ex_mover; uint8_t* ex_act; int32_t* ex_len; int8_t* ex_winner;
    u32* root_N; float *root_W, *root_P;
    u64* counters; u64* cnt_slots; int n_cnt_slots; u32* flags;
    int32_t* pack_off;  // [rounds][B]: first row of a finished game in the packed example block (k_pack_scan)
    // evaluation cache (BZ_ENGINE_EVAL_CACHE, net evaluators): per game a hash table position -> node of its first
    // evaluation in the current search (tt_buckets buckets of 16 eight-byte entries) and every node's value
    // ecache == 2 (BZ_ENGINE_EVAL_CACHE_CARRY): the previous search's tree stays intact in the other arena (nodes_alt / edges_alt
    // / node_v_alt: the arenas alternate search by search) and its evaluations serve this search too
    int ecache, tt_buckets; u64* tt; float *node_v, *node_v_alt;
};

// Gumbel root search (m = 0: off), set by bz_engine_set_gumbel in the caller's buffer: the considered-visit
// table T [m][sims] (row n_c - 1), every root edge's base = g + logf(P~) [B][MAXCH] and the root's value v_root [B].  A kernel
// argument of the Gumbel kernels only: EngineDev, and with it every other kernel's code, stays what it is.
struct GumbelDev {
    int m; float scale, mvi, vs;
    const uint16_t* T; float *base, *vroot;
};

// Playout cap randomisation (fast = 0: off), set by bz_engine_set_playout_cap: every slot's simulation budget
// for the current search, b_g [B] in the caller's buffer (k_cap_budget writes it behind k_root_begin; 0 = the slot sits the
// search out).  Like GumbelDev a kernel argument of the cap kernels only.
struct CapDev {
    int fast; u32 full_q;
    u32* budget;
};
constexpr u64 kCapKey = 0x706C61796F757443ULL;
// the budget draw: all-integer, so the host (bz_playout_cap_budget), the kernel and the twin agree on every bit
__host__ __device__ __forceinline__ u32 cap_budget(u64 seed, u64 gid, u64 made, int sims, int fast, u32 full_q) {
    return (u32)(rng_draw(seed ^ kCapKey, gid, made) & 0xFFFFULL) < full_q ? (u32)sims : (u32)fast;
}

// Forced playouts and policy target pruning (k = 0: off), set by bz_engine_set_forced_playouts.  Like CapDev a
// kernel argument of the forced kernels only.
struct ForcedDev { float k; int prune; };
// n_forced of a root edge with prior P at the root's child visit sum sumN
__host__ __device__ __forceinline__ float forced_nf(float k, float P, u32 sumN) {
    float t = k * P;
    t = t * (float)sumN;
    return fsqrt(t);
}
// the DESIGN.md 3.3 score of an edge with mean value q and prior P at Nf visits
__host__ __device__ __forceinline__ float puct_score(float q, float c_puct, float P, float sq, float Nf) {
    float u = c_puct * P;
    u = u * sq;
    u = fdiv(u, 1.0f + Nf);
    return q + u;
}
// Policy target pruning over the root's n edges: sink(i, edge, N') for every edge in ascending order, the sum
// of the N' returned.  The kernels (sink: the pi row) and bz_forced_prune (sink: N_out) run this one function.
template <class Sink>
__host__ __device__ __forceinline__ u32 forced_prune(const Edge* ed, int n, float c_puct, float k, Sink&& sink) {
    u32 sumN = 0, bn = 0;
    int cs = 0;
    for (int i = 0; i < n; ++i) {
        const u32 N = e_N(ed[i].w0);
        sumN += N;
        if (N > bn) { bn = N; cs = i; }
    }
    const float sq = fsqrt((float)(sumN > 1u ? sumN : 1u));
    float ss = 0.0f;
    if (n > 0) {
        const Edge b = ed[cs];
        ss = puct_score(bn > 0 ? fdiv(b.W, (float)bn) : 0.0f, c_puct, b.P, sq, (float)bn);
    }
    u32 sum2 = 0;
    for (int i = 0; i < n; ++i) {
        const Edge e = ed[i];
        const u32 N = e_N(e.w0);
        u32 Np = N;
        if (i != cs && N > 0) {
            const float nf = forced_nf(k, e.P, sumN);
            const u32 lim = !(nf < (float)N) ? N : (u32)__builtin_ceilf(nf);  // min(m, N), m the smallest integer >= nf
            const float q = fdiv(e.W, (float)N);
            for (u32 t = 1; t <= lim; ++t) {
                if (!(puct_score(q, c_puct, e.P, sq, (float)(N - t)) < ss)) break;
                Np = N - t;
            }
            if (Np < N && Np <= 1u) Np = 0;
        }
        sink(i, e, Np);
        sum2 += Np;
    }
    return sum2;
}

// Policy surprise weighting (prior = nullptr: off), set by bz_engine_set_surprise in the caller's buffer: every
// root's raw prior [B][MAXCH] in edge order as the expansion stored it (k_surp_save, before any noise), the row the play
// kernel is about to write per slot (row + 1; 0 = none) and the rows' kl [rounds][B][t_max].  A kernel argument of the
// surprise kernels only: the feature observes, no other kernel's code changes.
struct SurpDev { float* prior; u64* pend; float* ex_kl; };
// Search-value targets (ex_q = nullptr: off), set by bz_engine_set_search_value in the caller's buffer: the root's
// search value of every recorded row, f32 [rounds][B][t_max] indexed like ex_pi.  Read and written by the two value kernels only.
struct ValueDev { float* ex_q; };
// First-play urgency reduction (root_w = nullptr: off), set by bz_engine_set_fpu: the two reductions and every
// root's running value sum Wr f32 [B] in the caller's buffer.  A kernel argument of the FPU kernels only.
struct FpuDev { float reduction, root_reduction; float* root_w; };
// Gumbel interior selection (node_v = nullptr: off), set by bz_engine_set_gumbel_interior in the caller's buffer:
// the value every node of the current search was expanded with, f32 [B][ncap] indexed like the nodes.  A kernel argument of
// k_gfull_step only.
struct GumbelInDev { float* node_v; };
// Ownership targets (fin_x = nullptr: off), set by bz_engine_set_ownership in the caller's buffer: every finished
// game's final board in absolute colours, u64 [rounds][B] each, indexed like ex_len, and the scratch the root-policy kernel
// writes in front of the play kernel (pi [B][NA], act [B]).  A kernel argument of the two ownership kernels only.
struct OwnDev { u64 *fin_x, *fin_o; float* pi; int32_t* act; };

// Proven wins, losses and draws (root = nullptr: off), set by bz_engine_set_solver in the caller's buffer: every
// root's proven value + 2 (0 = undecided) i32 [B] and the two counts of the current search -- nodes newly decided, walks that
// ended at a proven edge that is not terminal.  bz_engine_root_begin zeroes all of it.  A kernel argument of the solver kernels only.
struct SolveDev { int32_t* root; u32* counts; };

// Resignation (streak = nullptr: off), set by bz_engine_set_resign in the caller's buffer: every game's two
// streaks u8 [rounds][B][2] (side +1, side -1) and its record -- the side that fired first i8 (0: none), the moves made and the
// root value at that search, and whether the game is played out u8 -- [rounds][B] each, indexed like ex_len.  A kernel argument
// of the two resignation kernels only.
struct ResignDev { float threshold; int consecutive; u32 playout_q; uint8_t* streak; int8_t* side; int32_t* move; float* q; uint8_t* played_out; };
// g_state of a slot k_resign_note has ended and k_resign_finish has not yet restarted or retired: like every value but 0 it
// makes the kernels between the two skip the slot
constexpr uint8_t kStateResigned = 2;
// Exact early stop (stop_at = nullptr: off), set by bz_engine_set_early_stop in the caller's buffer: the simulation
// index every slot stopped at in the current search u32 [B] (sims: it ran its whole budget; 0: it sat the search out) and one
// word, walked = 1 + the index of the last tree step in which some slot walked.  k_stop_begin resets both behind k_root_begin.  A
// kernel argument of the stop kernels only.
struct StopDev { u32* stop_at; u32* walked; };

// ---- The search mode (kMode*, csrc/bz_options.h): one compile-time mask M per kernel
// the mask's bits by name, and the combinations no code serves: mode_served asks the table the setters (bz_engine_set_*) refuse
// from at run time
template <unsigned M>
struct Mode {
    static constexpr bool leaf = (M & kModeLeaf) != 0, gumbel = (M & kModeGumbel) != 0, cap = (M & kModeCap) != 0,
                          forced = (M & kModeForced) != 0, fpu = (M & kModeFpu) != 0, gfull = (M & kModeGfull) != 0,
                          solve = (M & kModeSolve) != 0, stop = (M & kModeStop) != 0, pace = (M & kModePace) != 0;
    static_assert(!gfull || gumbel, "search mode: the Gumbel interior rule needs Gumbel root search");
    static_assert(mode_served(M), "search mode: two of its options are a refused pair (kConflicts, csrc/bz_options.h)");
    static_assert(!pace || M == kModePace, "search mode: the paced step serves the plain search only");
};
// what the modes' kernels get beside EngineDev: each pointer is read only under its bit and stays null otherwise
struct ModeArgs {
    const GumbelDev* gm = nullptr;    // kModeGumbel
    const u32* budget = nullptr;      // kModeCap: b_g [B]
    const ForcedDev* fo = nullptr;    // kModeForced
    const FpuDev* fp = nullptr;       // kModeFpu
    const GumbelInDev* gi = nullptr;  // kModeGfull
    const SolveDev* sv = nullptr;     // kModeSolve
    const StopDev* sp = nullptr;      // kModeStop
};

struct Cnt { u32 v[CNT_N]; };

// Diagnostic build only (betazero_amd.build.build_variant("treestamps", ["-DBZ_EXP_TREE_STAMPS"]), tools/exp_tree_stamps.py):
// shader-clock stamps between the phases of k_tree_step, summed over all waves into counters[16..23].  The product build
// compiles the empty struct away.
#ifdef BZ_EXP_TREE_STAMPS
struct Stamps {
    u64 last; u32 acc[8];
    __device__ __forceinline__ void start() { for (int k = 0; k < 8; ++k) acc[k] = 0; last = __builtin_readcyclecounter(); }
    __device__ __forceinline__ void mark(int k) { const u64 now = __builtin_readcyclecounter(); acc[k] += (u32)(now - last); last = now; }
    __device__ __forceinline__ void flush(u64* counters) {
        if ((threadIdx.x & 63) == 0) {
            for (int k = 0; k < 7; ++k) atomicAdd(reinterpret_cast<unsigned long long*>(counters) + 16 + k, (unsigned long long)acc[k]);
            atomicAdd(reinterpret_cast<unsigned long long*>(counters) + 23, 1ULL);  // waves
        }
    }
};
#else
struct Stamps {
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void flush(u64*) {}
};
#endif

// ---- lane exchange inside a lane group (kGW <= 16 lanes = at most one DPP row): butterfly partner for step O,
// valid when the steps run in ASCENDING order (1, 2, 4, 8): 1 and 2 are quad permutes, 4 / 8 the half-row / row
// mirrors (the lower levels are uniform by then, so the mirror image is the partner half).  DPP moves are VALU
// operations; the ds_bpermute a generic shuffle compiles to is an LDS round trip.
template <int O>
__device__ __forceinline__ int xchg_i(int x) {
    static_assert(O == 1 || O == 2 || O == 4 || O == 8, "butterfly step");
    constexpr int ctrl = O == 1 ? 0xB1 : (O == 2 ? 0x4E : (O == 4 ? 0x141 : 0x140));
    return __builtin_amdgcn_update_dpp(0, x, ctrl, 0xF, 0xF, true);
}
template <int O> __device__ __forceinline__ u32 xchg(u32 x) { return (u32)xchg_i<O>((int)x); }
template <int O> __device__ __forceinline__ int xchg(int x) { return xchg_i<O>(x); }
template <int O> __device__ __forceinline__ float xchg(float x) { return __int_as_float(xchg_i<O>(__float_as_int(x))); }
// value of the previous lane of the row (lane 0 of a row: 0)
__device__ __forceinline__ float row_shr1(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x111, 0xF, 0xF, true));
}

// PUCT candidates: first maximum (lowest child index on ties) over the kGW lanes of a group
struct Cand { float sc; int i; u32 w0, w3; float W; };
template <int O>
__device__ __forceinline__ void cand_step(Cand& c) {
    const float s2 = xchg<O>(c.sc), W2 = xchg<O>(c.W); const int i2 = xchg<O>(c.i);
    const u32 a2 = xchg<O>(c.w0), b2 = xchg<O>(c.w3);
    const bool take = (s2 > c.sc) || (s2 == c.sc && i2 < c.i);
    if (take) { c.sc = s2; c.i = i2; c.w0 = a2; c.w3 = b2; c.W = W2; }
}
template <int kGW>
__device__ __forceinline__ void group_argmax(Cand& c) {
    if (kGW > 1) cand_step<1>(c);
    if (kGW > 2) cand_step<2>(c);
    if (kGW > 4) cand_step<4>(c);
    if (kGW > 8) cand_step<8>(c);
}
template <int kGW>
__device__ __forceinline__ float group_max(float m) {
    if (kGW > 1) { float m2 = xchg<1>(m); m = m2 > m ? m2 : m; }
    if (kGW > 2) { float m2 = xchg<2>(m); m = m2 > m ? m2 : m; }
    if (kGW > 4) { float m2 = xchg<4>(m); m = m2 > m ? m2 : m; }
    if (kGW > 8) { float m2 = xchg<8>(m); m = m2 > m ? m2 : m; }
    return m;
}
template <int kGW>
__device__ __forceinline__ float group_min(float m) {
    if (kGW > 1) { float m2 = xchg<1>(m); m = m2 < m ? m2 : m; }
    if (kGW > 2) { float m2 = xchg<2>(m); m = m2 < m ? m2 : m; }
    if (kGW > 4) { float m2 = xchg<4>(m); m = m2 < m ? m2 : m; }
    if (kGW > 8) { float m2 = xchg<8>(m); m = m2 < m ? m2 : m; }
    return m;
}
template <int kGW>
__device__ __forceinline__ u32 group_max_u32(u32 m) {
    if (kGW > 1) { u32 m2 = xchg<1>(m); m = m2 > m ? m2 : m; }
    if (kGW > 2) { u32 m2 = xchg<2>(m); m = m2 > m ? m2 : m; }
    if (kGW > 4) { u32 m2 = xchg<4>(m); m = m2 > m ? m2 : m; }
    if (kGW > 8) { u32 m2 = xchg<8>(m); m = m2 > m ? m2 : m; }
    return m;
}
// SEQUENTIAL float sum over the kGW lanes of a group in ascending lane order (Gumbel interior rule): returns
// ((carry + x_0) + x_1) + ... + x_{kGW-1} in every lane, each addition one rounding, left to right -- the bits of the serial loop.
// A systolic pass: in every step each lane adds its x to what the lane before it holds (lane 0: to the carry), so after step s
// the lanes 0 .. s hold their final prefix and recompute the same value from then on; kGW steps of one DPP move and one add.
// A lane without a term passes x = +0.0f: the running sum starts from +0.0f and is therefore never -0.0f, so the addition
// changes no bit.  (The DPP shift crosses into the neighbouring group only in lane 0, whose input is replaced by the carry.)
template <int kGW>
__device__ __forceinline__ float group_seq_sum(float carry, float x, int sub) {
    float acc = 0.0f;
#pragma unroll
    for (int s = 0; s < kGW; ++s) {
        float t = row_shr1(acc);
        t = sub == 0 ? carry : t;
        acc = t + x;
    }
    return __shfl(acc, kGW - 1, kGW);
}
// integer sum over the kGW lanes of a group (first-play urgency): whatever the order, the same bits
template <int kGW>
__device__ __forceinline__ u32 group_sum_u32(u32 x) {
    if (kGW > 1) x += xchg<1>(x);
    if (kGW > 2) x += xchg<2>(x);
    if (kGW > 4) x += xchg<4>(x);
    if (kGW > 8) x += xchg<8>(x);
    return x;
}

// OR over the kGW lanes of a group (the solver's node rule)
template <int kGW>
__device__ __forceinline__ u32 group_or_u32(u32 x) {
    if (kGW > 1) x |= xchg<1>(x);
    if (kGW > 2) x |= xchg<2>(x);
    if (kGW > 4) x |= xchg<4>(x);
    if (kGW > 8) x |= xchg<8>(x);
    return x;
}

// counters are accumulated by the lead lane of every lane group and flushed per wave into that wave's own slot
// (1000+ waves hammering 8 shared addresses cost more than the tree walk itself): the leads' counts are summed
// across the groups, then lanes 0..7 each add ONE counter with an atomic that returns nothing -- nothing waits
// for it (eight load -> wait -> store sequences at the end of every wave were a fifth of the tree step's time).
// k_sum_counters folds the slots into counters[16] when the host asks.
template <int kGW>
__device__ __forceinline__ void cnt_flush(const EngineDev& E, Cnt& c) {
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = (int)(threadIdx.x & 63);
    u32 mine = 0;
#pragma unroll
    for (int k = 0; k < CNT_N; ++k) {
        u32 x = c.v[k];
        if (kGW >= 16) {  // few leads (lanes 0, kGW, ...): read them straight into scalar registers -- no LDS round trips
            u32 sum = 0;
#pragma unroll
            for (int l = 0; l < 64; l += kGW) sum += (u32)__builtin_amdgcn_readlane((int)x, l);
            x = sum;
        } else {
#pragma unroll
            for (int o = 32; o >= kGW; o >>= 1) x += __shfl_xor(x, o, 64);  // (lanes that are not leads hold zeros)
            x = (u32)__builtin_amdgcn_readfirstlane((int)x);                 // lane 0 is a lead: it holds the wave's sum
        }
        mine = lane == k ? x : mine;
    }
    if (lane < CNT_N && mine && wave < (u32)E.n_cnt_slots)
        __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(E.cnt_slots) + (size_t)wave * CNT_N + lane,
                               (unsigned long long)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) k_sum_counters(EngineDev E) {
    __shared__ unsigned long long part[256];
    for (int k = 0; k < CNT_N; ++k) {
        unsigned long long acc = 0;
        for (int w = threadIdx.x; w < E.n_cnt_slots; w += 256) acc += E.cnt_slots[(size_t)w * CNT_N + k];
        part[threadIdx.x] = acc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o]; __syncthreads(); }
        if (threadIdx.x == 0) E.counters[k] = part[0];
        __syncthreads();
    }
}

// Orders a lane group's earlier stores (edges / node header written by dev_expand, child node
// written by dev_select) before its later loads of the same addresses.  All communication is
// between lanes of ONE wave (a game's G::GW lanes divide 64), so WAVEFRONT scope is the exact
// scope: acq_rel keeps the compiler from moving the stores or the following loads across it,
// and the hardware executes one wave's vector-memory instructions to an address in issue order,
// so no s_waitcnt vmcnt(0) (a full store round trip, which a workgroup-scope fence costs) is needed.
__device__ __forceinline__ void group_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// where the select walk records its path: edge index + that edge's w0 (N and the child header) and W as the walk
// saw / left them, so that the backup is a pure store.  HBM, game-major (a game's entries are one coalesced load for
// its lane group), for the step-by-step kernels whose backup runs in the next launch; LDS for the fused search.
// (every lane of the group calls put() with the same arguments)
template <int kGW>
struct PathHbm {  // lane d of the group keeps entry d in registers during the walk -- no store, so nothing for the next
    PathEnt* p;   // level's load to queue behind -- and writes it at the end (one coalesced store per game); levels
    PathEnt mine; // beyond the group width (rare) go to memory directly
    __device__ __forceinline__ void put(int d, int sub, u32 eidx, u32 w0, float W) {
        if (d < kGW) { if (sub == d) { mine.eidx = eidx; mine.w0 = w0; mine.W = W; } }
        else if (sub == 0) { PathEnt e; e.eidx = eidx; e.w0 = w0; e.W = W; e.pad = 0; p[d] = e; }
    }
    __device__ __forceinline__ void flush(int sub, int depth) const { if (sub < depth && sub < kGW) p[sub] = mine; }
};
struct PathEntLds { u32 eidx; u32 w0; float W; };  // 12 bytes: LDS capacity decides how many games a CU holds
struct PathLds {
    PathEntLds* p;  // this game's MAXD entries
    __device__ __forceinline__ void put(int d, int sub, u32 eidx, u32 w0, float W) const {
        if (sub == 0) { PathEntLds e; e.eidx = eidx; e.w0 = w0; e.W = W; p[d] = e; }
    }
};

// logits source for the expansion of one leaf
struct LogitSrc {
    int kind; u64 h; const float* row;
    __device__ __forceinline__ float operator()(int a) const {
        return kind == BZ_EVAL_UNIFORM ? 0.0f : (kind == BZ_EVAL_HASH ? hash_logit(h, a) : row[a]);
    }
};

// ---- cooperative tree walk: G::GW lanes serve one game (Reversi 16 -> 4 games per wave, TTT 4 -> 16
// games per wave: the walk is a dependent chain per game, so games in flight = memory-level
// parallelism).  A level of the PUCT walk is one coalesced 256-byte load of up to 16 edges (the chosen
// edge's words say where the child's edges are, how many, and whether the child is terminal), the
// scores are computed one child per lane and reduced with 4 shuffle steps (first maximum, i.e.
// lowest action on ties); softmax terms are computed one legal move per lane, but SUMMED in
// ascending action order by a serial shuffle scan so that the result is bit-identical to the
// sequential spec; the backup updates one path edge per lane.

// ---- the env step of child creation, shared out over a lane group.  All kGW lanes of a group would otherwise
// compute the same 8 rays of make_move (reversi_board.py:49-58) and the same 8 rays of the child's legal mask
// (:25-41, :87-88) redundantly -- ~400 integer instructions per wave, on the walk's critical path.  Instead lane
// (sub & 7) takes ONE ray direction: directions 0..3 shift left by 1 / 8 / 7 / 9; 4..7 are their opposites,
// computed as the same left shifts on the bit-reversed boards (bit i <-> 63 - i maps a right shift onto a left
// shift; the column-wrap mask is symmetric), and the 8 partial masks are OR-ed across the lanes with DPP moves.
__device__ __forceinline__ u64 brev64(u64 x) { return ((u64)__brev((u32)x) << 32) | (u64)__brev((u32)(x >> 32)); }
__device__ __forceinline__ u64 or8(u64 x) {  // OR over the 8 lanes of a half row (lanes 8..15 of a 16-lane group mirror 0..7)
    u32 lo = (u32)x, hi = (u32)(x >> 32);
    lo |= xchg<1>(lo); hi |= xchg<1>(hi);
    lo |= xchg<2>(lo); hi |= xchg<2>(hi);
    lo |= xchg<4>(lo); hi |= xchg<4>(hi);
    return ((u64)hi << 32) | lo;
}
// one ray direction (left shift by s) of generate_possible_moves / of the flips of placing on m; o = opponent
// stones pre-masked against column wrap; runs of <= 6 stones by parallel prefix (2 + 2 + 2 cells)
__device__ __forceinline__ u64 ray_fill(u64 seed, u64 o, int s) {
    u64 fl = o & (seed << s);
    fl = and_or(o, fl << s, fl);
    const u64 pl = o & (o << s);
    fl = and_or(pl, fl << (2 * s), fl);
    fl = and_or(pl, fl << (2 * s), fl);
    return fl;
}
template <class G, bool kShare = (G::kGame != 0 && G::GW >= 8)>
struct CoopChild {  // tic-tac-toe / narrow groups: nothing to share out
    static __device__ __forceinline__ void run(u64 own, u64 opp, int act, int, u64* cown, u64* copp, u64* legal) {
        G::apply(own, opp, act, cown, copp);
        *legal = G::legal(*cown, *copp);
    }
};
template <class G>
struct CoopChild<G, true> {
    static __device__ __forceinline__ void run(u64 own, u64 opp, int act, int sub, u64* cown, u64* copp, u64* legal) {
        const int d = sub & 7, k = d & 3;
        const int s = k == 0 ? 1 : (k == 1 ? 8 : (k == 2 ? 7 : 9));
        const bool rv = d >= 4;
        const u64 wrap = k == 1 ? ~0ULL : kInner;
        u64 co = opp, cp = own;
        if (act != kPass) {
            const u64 m = 1ULL << act;
            const u64 a = rv ? brev64(own) : own, b = rv ? brev64(opp) : opp, mm = rv ? brev64(m) : m;
            u64 fl = ray_fill(mm, b & wrap, s);
            fl = ((fl << s) & a) ? fl : 0ULL;
            const u64 f = or8(rv ? brev64(fl) : fl);
            co = opp & ~f; cp = own | m | f;
        }
        const u64 a = rv ? brev64(co) : co, b = rv ? brev64(cp) : cp;
        const u64 mv = ray_fill(a, b & wrap, s) << s;
        *legal = or8(rv ? brev64(mv) : mv) & ~(co | cp) & G::kValid;
        *cown = co; *copp = cp;
    }
};

// what the walk starts from: the root's position, mover colour and child count (its edges start at index 0)
// `pre`: this lane's root edge (index sub) when the caller fetched the first kGW root edges ahead of the walk
struct RootRef { u64 own, opp; int tm; int n; u32 sumN; bool has_pre; Edge pre; u32 tt_gen, prev_nodes; };
// the node select created (valid when a child was created); src / src_e0: the node whose evaluation a COPY leaf shares
struct LeafPos { u64 own, opp, legal; u32 info, src, src_e0; };

// ---- evaluation cache.  A search reaches some positions by more than one move order (measured on the CPU oracle: 6 - 12 %
// of the 800 evaluations of a cfg-3 search, profiles/r05_leaf_duplication.json); the net is a function of the position
// alone, so the second node takes the first one's priors and value -- bit for bit what the evaluator would have returned
// -- and no evaluator row.  The TREE is unchanged: the repeat is a node of its own with its own statistics (exact
// sequential MCTS, the oracle's tree), only the evaluation is shared.  Per game a table of tt_buckets x 16 entries
// {tag 32 | generation 19 | node 13}; the bucket is one coalesced 128-byte load by the game's lanes; a tag match is
// CONFIRMED against the stored node's position (a false positive is impossible, whatever the hash does); entries of
// earlier searches (other generation) are free slots; a full bucket just means no insertion.
constexpr u32 kTtGenMax = (1u << 19) - 1u;
template <int kGW>
__device__ __forceinline__ u32 group_min_u32(u32 x) {
    if (kGW > 1) { const u32 y = xchg<1>(x); x = y < x ? y : x; }
    if (kGW > 2) { const u32 y = xchg<2>(x); x = y < x ? y : x; }
    if (kGW > 4) { const u32 y = xchg<4>(x); x = y < x ? y : x; }
    if (kGW > 8) { const u32 y = xchg<8>(x); x = y < x ? y : x; }
    return x;
}
// looks (own, opp) up.  A confirmed hit returns true with the source node -- flagged kSrcPrev when it is a node of the
// PREVIOUS search's tree (carry-over: generation gen - 1, arena nodes_alt, only ids below prev_nodes) -- and its first edge.
// A miss, and a carry-over hit too, inserts `new_id` for this generation (nodes 0 .. new_id - 1 of this search exist and are
// expanded; the new node will be by the time anyone finds it).  All lanes of the group return the same values.
template <int kGW>
__device__ __forceinline__ bool tt_lookup_insert(const EngineDev& E, int g, int sub, u64 own, u64 opp, u32 gen, u32 prev_nodes,
                                                 u32 new_id, u32& src, u32& src_e0) {
#ifdef BZ_EXP_TT_WEAK_HASH
    // TEST BUILD ONLY (tests/test_gpu_parity.py): every position has tag 0 and lives in one of two buckets -- tag matches that
    // are NOT the position and full buckets become the normal case; the results must still be those without any cache
    const u64 h = hash_pos(own, opp) & 1u;
#else
    const u64 h = hash_pos(own, opp);
#endif
    const u32 tag = (u32)(h >> 32);
    const u32 gen_prev = gen == 1u ? kTtGenMax - 1u : gen - 1u;  // (the host's counter cycles 1 .. 2^19 - 2)
    u64* bucket = E.tt + ((size_t)g * (size_t)E.tt_buckets + (size_t)(h & (u64)(E.tt_buckets - 1))) * 16;
    // (is-previous << 20 | slot << 16 | node) of the best matching slot this lane saw: this search's entries win
    u32 hit = ~0u, fre = ~0u;
#pragma unroll
    for (int s0 = 0; s0 < 16; s0 += kGW) {
        const int s = s0 + sub;
        const u64 e = bucket[s];
        const u32 meta = (u32)(e >> 32), egen = meta >> kChildBits;
        const bool cur = egen == gen, prv = prev_nodes != 0u && egen == gen_prev;
        if ((cur || prv) && (u32)e == tag) {
            const u32 key = ((prv ? 1u : 0u) << 20) | ((u32)s << 16) | (meta & kChildMask);
            hit = key < hit ? key : hit;
        }
        if (!cur && !prv && fre == ~0u) fre = (u32)s << 16;
    }
    hit = group_min_u32<kGW>(hit);
    fre = group_min_u32<kGW>(fre);
    bool found = false, from_prev = false;
    if (hit != ~0u) {
        const u32 x = hit & kChildMask;
        from_prev = (hit >> 20) != 0u;
        if (x != 0u && x < (from_prev ? prev_nodes : new_id)) {
            const Node xn = (from_prev ? E.nodes_alt : E.nodes)[(size_t)g * E.ncap + x];  // (one address for the whole group)
            found = xn.own == own && xn.opp == opp && !(xn.info & kTerm) && (xn.info & 0xFFu) != 0u;
            src = x | (from_prev ? kSrcPrev : 0u); src_e0 = xn.edge0;
        }
    }
    if ((!found || from_prev) && fre != ~0u) {
        const int s = (int)(fre >> 16);
        if (sub == s % kGW) bucket[s] = (u64)tag | ((u64)((gen << kChildBits) | new_id) << 32);
    }
    return found;
}

// ---- Gumbel root search.  Every expression is one binary32 operation in the written order; sums run
// over the root's edges in ascending order.  These helpers are serial loops over the root's <= 34 edges: in the tree step
// every lane of the game's group runs the same loop on the same (broadcast) loads, so all lanes agree without exchanges.
constexpr float kFltMin = 1.17549435e-38f;  // 2^-126
__device__ __forceinline__ float gumbel_pfloor(float P) { return P > kFltMin ? P : kFltMin; }
// what sigma(completed Q) needs from the root's current statistics: cq_i = N_i > 0 ? W_i / N_i : vmix,
// sigma_i = s * ((cq_i - lo) / d)
struct GumbelStats { float vmix, lo, d, s; u32 nmax; };
__device__ __forceinline__ float gumbel_cq(const Edge& e, float vmix) {
    const u32 N = e_N(e.w0);
    return N > 0 ? fdiv(e.W, (float)N) : vmix;
}
__device__ __forceinline__ float gumbel_sigma(const GumbelStats& st, float cq) { return st.s * fdiv(cq - st.lo, st.d); }
__device__ __forceinline__ GumbelStats gumbel_stats(const GumbelDev& Gm, const Edge* ed, int n, float v_root) {
    u32 S = 0, nmax = 0;
    float sp = 0.0f, spq = 0.0f;
    for (int i = 0; i < n; ++i) {
        const Edge e = ed[i];
        const u32 N = e_N(e.w0);
        S += N;
        nmax = N > nmax ? N : nmax;
        if (N > 0) {
            const float q = fdiv(e.W, (float)N), pf = gumbel_pfloor(e.P);
            sp = sp + pf;
            const float t = pf * q;
            spq = spq + t;
        }
    }
    const float wq = sp > 0.0f ? fdiv(spq, sp) : 0.0f;
    GumbelStats st;
    if (S == 0) {
        st.vmix = v_root;
    } else {
        const float t = (float)S * wq;
        const float a = v_root + t;
        const float b = (float)S + 1.0f;
        st.vmix = fdiv(a, b);
    }
    float lo = 0.0f, hi = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float cq = gumbel_cq(ed[i], st.vmix);
        lo = (i == 0 || cq < lo) ? cq : lo;
        hi = (i == 0 || cq > hi) ? cq : hi;
    }
    float d = hi - lo;
    st.d = d < 1e-8f ? 1e-8f : d;
    st.lo = lo;
    float s = Gm.mvi + (float)nmax;
    st.s = s * Gm.vs;
    st.nmax = nmax;
    return st;
}
// the root edge a walk takes at the root's visit sum k: among the edges with N == T[n_c][k], the first maximum of base + sigma
// (one exists by construction of T; edge 0 stands in if the statistics were ever not those of this search)
template <class G>
__device__ __forceinline__ int gumbel_root_pick(const EngineDev& E, const GumbelDev& Gm, int g, const Edge* ed, int n, u32 k) {
    if (n <= 0) return 0;  // (a root without edges: nothing to choose, as in the PUCT loop)
    const int nc = n < Gm.m ? n : Gm.m;
    const u32 kk = k < (u32)E.sims ? k : (u32)E.sims - 1u;
    const u32 cv = Gm.T[(size_t)(nc - 1) * E.sims + kk];
    const GumbelStats st = gumbel_stats(Gm, ed, n, Gm.vroot[g]);
    const float* base = Gm.base + (size_t)g * G::MAXCH;
    int best = -1;
    float bests = 0.0f;
    for (int i = 0; i < n; ++i) {
        const Edge e = ed[i];
        if (e_N(e.w0) != cv) continue;
        const float sc = base[i] + gumbel_sigma(st, gumbel_cq(e, st.vmix));
        if (best < 0 || sc > bests) { best = i; bests = sc; }
    }
    return best < 0 ? 0 : best;
}

// M2: PUCT walk from the root; creates the child node behind the chosen unexpanded edge (env step:
// apply + legal + terminal).  All lanes of the group return the same values.  M: the search mode (Mode, above); beside A the
// two values that differ walk by walk: fk, the slot's forced parameter in this search (kModeForced; 0 = it does not force), and
// Wr, the root's running value sum as of this walk (kModeFpu).
template <class G, unsigned M, class Sink>
__device__ __forceinline__ void dev_select(const EngineDev& E, int g, int sub, const RootRef& root, u32& n_nodes_g,
                                           u32& leaf, int& kind, int& depth_out, float& tval, Cnt& c,
                                           Sink& sink, LeafPos& lp, Stamps& st, const ModeArgs& A, float fk, float Wr) {
    constexpr bool kLeafPar = Mode<M>::leaf, kGumbel = Mode<M>::gumbel, kForced = Mode<M>::forced, kFpu = Mode<M>::fpu,
                   kGfull = Mode<M>::gfull, kSolve = Mode<M>::solve;
    constexpr int kGW = G::GW;
    constexpr int kCH = (G::MAXCH + kGW - 1) / kGW;
    [[maybe_unused]] float vx = 0.0f;  // kGfull: v_X of the node whose edges are being scored (depth >= 1) ...
    [[maybe_unused]] const float* gnv = nullptr;  // ... from this game's row of the interior buffer
    if constexpr (kGfull) gnv = A.gi->node_v + (size_t)g * E.ncap;
    // kFpu: the value of the node whose edges are being scored -- the root's Wr / simulations so far, 0 before the first
    float qx = 0.0f;
    if (kFpu) qx = root.sumN > 0u ? fdiv(Wr, (float)root.sumN) : 0.0f;
    Node* nodes = E.nodes + (size_t)g * E.ncap;
    Edge* edges = E.edges + (size_t)g * E.ecap;
    // sum of the root's child visits == simulations done so far (+ the visits a kept subtree came with)
    u32 e0 = 0, sumN = root.sumN;
    int n = root.n, depth = 0;
    u64 pown = root.own, popp = root.opp;  // position of the node whose edges are being scored
    const bool lead = sub == 0;
    if (lead) { c.v[CNT_SIMS]++; c.v[CNT_PATH_NODES]++; }
    for (;;) {
        const float sq = fsqrt((float)(sumN > 1u ? sumN : 1u));
        const Edge* ed = edges + e0;
        float bests = -__builtin_inff(), bestW = 0.0f; int best = 0; u32 bestw0 = 0, bestw3 = 0;
        if (kGumbel && depth == 0) {  // (the root's edges start at index 0; sumN = the root's visit sum = sim_index)
            best = gumbel_root_pick<G>(E, *A.gm, g, ed, n, sumN);
            const Edge e = ed[best];
            bestw0 = e.w0; bestw3 = e.w3; bestW = e.W;
        } else if (kGfull) {  // (depth >= 1: X is expanded and not terminal)
            Edge ev[kCH];
#pragma unroll
            for (int k = 0; k < kCH; ++k) {
                const int i = k * kGW + sub;
                ev[k].w0 = 0; ev[k].W = 0.0f; ev[k].P = 0.0f; ev[k].w3 = 0;
                if (i < n) ev[k] = ed[i];
            }
            if (n <= 1) {  // a forced pass: edge 0 (lane 0 holds it)
                best = 0;
                bestw0 = (u32)__shfl((int)ev[0].w0, 0, kGW); bestw3 = (u32)__shfl((int)ev[0].w3, 0, kGW);
                bestW = __shfl(ev[0].W, 0, kGW);
            } else {
                // ---- statistics: q one edge per lane, sp / spq sequentially in edge order, nmax by a group reduction
                float cq[kCH];
                float sp = 0.0f, spq = 0.0f;
                u32 nmax = 0;
#pragma unroll
                for (int k = 0; k < kCH; ++k) {
                    const u32 N = e_N(ev[k].w0);  // (0 in a lane without an edge)
                    const bool vis = N > 0u;
                    const float q = vis ? fdiv(ev[k].W, (float)N) : 0.0f, pf = gi_pfloor(ev[k].P);
                    const float t = pf * q;
                    cq[k] = q;
                    nmax = N > nmax ? N : nmax;
                    if (k * kGW < n) {  // (the same for the whole group)
                        sp = group_seq_sum<kGW>(sp, vis ? pf : 0.0f, sub);
                        spq = group_seq_sum<kGW>(spq, vis ? t : 0.0f, sub);
                    }
                }
                nmax = group_max_u32<kGW>(nmax);
                const float vmix = gi_vmix(sumN, sp, spq, vx);
                float lo = __builtin_inff(), hi = -__builtin_inff();
#pragma unroll
                for (int k = 0; k < kCH; ++k) {
                    if (e_N(ev[k].w0) == 0u) cq[k] = vmix;
                    if (k * kGW + sub < n) { lo = cq[k] < lo ? cq[k] : lo; hi = cq[k] > hi ? cq[k] : hi; }
                }
                lo = group_min<kGW>(lo); hi = group_max<kGW>(hi);
                const GiScale gs = gi_scale(lo, hi, nmax, A.gm->mvi, A.gm->vs);
                // ---- the improved policy: x one edge per lane, the max by a group reduction, the sum sequentially
                float m = -__builtin_inff();
#pragma unroll
                for (int k = 0; k < kCH; ++k) {
                    cq[k] = gi_x(gs, ev[k].P, cq[k]);
                    if (k * kGW + sub < n) m = cq[k] > m ? cq[k] : m;
                }
                m = group_max<kGW>(m);
                float s = 0.0f;
#pragma unroll
                for (int k = 0; k < kCH; ++k) {
                    cq[k] = (k * kGW + sub < n) ? expf_spec(cq[k] - m) : 0.0f;
                    if (k * kGW < n) s = group_seq_sum<kGW>(s, cq[k], sub);
                }
                // ---- score and the first maximum: every lane's own over its <= kCH edges (ascending, strict >), then ONE reduction
                const float den = 1.0f + (float)sumN;
                Cand cd; cd.i = sub; cd.sc = -__builtin_inff(); cd.W = 0.0f; cd.w0 = 0; cd.w3 = 0;
#pragma unroll
                for (int k = 0; k < kCH; ++k) {
                    const int i = k * kGW + sub;
                    if (i < n) {
                        const Edge e = ev[k];
                        const float sc = gi_score(fdiv(cq[k], s), e_N(e.w0), den);
                        if (sc > cd.sc) { cd.sc = sc; cd.i = i; cd.w0 = e.w0; cd.w3 = e.w3; cd.W = e.W; }
                    }
                }
                group_argmax<kGW>(cd);
                best = cd.i; bestw0 = cd.w0; bestw3 = cd.w3; bestW = cd.W;
            }
        } else if (kFpu) {
            Edge ev[kCH];
            u32 S = 0;
#pragma unroll
            for (int k = 0; k < kCH; ++k) {
                const int i = k * kGW + sub;
                ev[k].w0 = 0; ev[k].W = 0.0f; ev[k].P = 0.0f; ev[k].w3 = 0;
                if (i < n) {
                    Edge e = root.pre;
                    if (!(root.has_pre && depth == 0 && k == 0)) e = ed[i];
                    ev[k] = e;
                    if (e_N(e.w0) > 0u) S += fpu_pq(e.P);
                }
            }
            S = group_sum_u32<kGW>(S);
            const float f = fpu_value(S, qx, depth == 0 ? A.fp->root_reduction : A.fp->reduction);
            // every lane's own first maximum over its <= kCH edges (ascending index, strict >), then ONE reduction over the group:
            // the first maximum over all edges, the lowest index on ties
            Cand cd; cd.i = sub; cd.sc = -__builtin_inff(); cd.W = 0.0f; cd.w0 = 0; cd.w3 = 0;
#pragma unroll
            for (int k = 0; k < kCH; ++k) {
                const int i = k * kGW + sub;
                if (i < n) {
                    const Edge e = ev[k];
                    const u32 N = e_N(e.w0);
                    const float q = N > 0 ? fdiv(e.W, (float)N) : f;
                    float sc = puct_score(q, E.c_puct, e.P, sq, (float)N);
                    if (kForced && depth == 0 && fk > 0.0f && N > 0 && (float)N < forced_nf(fk, e.P, sumN)) sc = __builtin_inff();
                    if (sc > cd.sc) { cd.sc = sc; cd.i = i; cd.w0 = e.w0; cd.w3 = e.w3; cd.W = e.W; }
                }
            }
            group_argmax<kGW>(cd);
            if (cd.sc > bests) { bests = cd.sc; best = cd.i; bestw0 = cd.w0; bestw3 = cd.w3; bestW = cd.W; }
        } else
        for (int base = 0; base < n; base += kGW) {
            Cand cd; cd.i = base + sub; cd.sc = -__builtin_inff(); cd.W = 0.0f; cd.w0 = 0; cd.w3 = 0;
            if (cd.i < n) {
                Edge e = root.pre;
                if (!(root.has_pre && depth == 0 && base == 0)) e = ed[cd.i];
                const u32 N = e_N(e.w0);
                float q = N > 0 ? fdiv(e.W, (float)N) : 0.0f;
                float u = E.c_puct * e.P;
                u = u * sq;
                u = fdiv(u, 1.0f + (float)N);
                if (kSolve && e_decided(e.w0) && e_val(e.w0) == 0) q = 0.0f;
                cd.sc = q + u; cd.w0 = e.w0; cd.w3 = e.w3; cd.W = e.W;
                if (kSolve && e_decided(e.w0) && e_val(e.w0) != 0) cd.sc = e_val(e.w0) < 0 ? __builtin_inff() : -__builtin_inff();
                if (kForced && depth == 0 && fk > 0.0f && N > 0 && (float)N < forced_nf(fk, e.P, sumN)) cd.sc = __builtin_inff();
            }
            group_argmax<kGW>(cd);
            // (kSolve: the first chunk's winner stands in until a higher score comes -- edge 0 when every edge scores -inf)
            if (cd.sc > bests || (kSolve && base == 0)) { bests = cd.sc; best = cd.i; bestw0 = cd.w0; bestw3 = cd.w3; bestW = cd.W; }
        }
        if (lead) c.v[CNT_CHILD_SCORED] += (u32)n;
        const u32 eidx = e0 + (u32)best;
        const u32 child = e_child(bestw3);
        if (child) {
            if (lead) c.v[CNT_PATH_NODES]++;
            if (depth < E.maxd) sink.put(depth, sub, eidx, bestw0, bestW);
            else if (lead) atomicOr(&E.flags[FLAG_ERR], ERR_DEPTH);
            depth++;
            if (kSolve ? e_decided(bestw0) : e_term(bestw0)) { kind = LEAF_TERMINAL; leaf = child; tval = (float)e_val(bestw0); break; }
            // leaf-parallel: a non-terminal child without edges was created by an earlier walk of this step
            if (kLeafPar && e_nch(bestw0) == 0) { kind = LEAF_COLLIDE; leaf = child; tval = 0.0f; break; }
            // children's visits of X == visits of the edge into X minus the creating one
            e0 = e_edge0(bestw3); n = e_nch(bestw0); sumN = e_N(bestw0) - 1u;
            if (kFpu) {  // X's value for its mover, from the edge the walk came in by (W is stored for the parent's mover; N >= 1)
                qx = fdiv(bestW, (float)e_N(bestw0));
                qx = -qx;
            }
            // X's position is needed only if the walk ends by extending X: the load goes out beside X's edge load
            const Node* xn = nodes + child;
            pown = xn->own; popp = xn->opp;
            if (kGfull) vx = gnv[child];  // (beside them: X's own value)
            continue;
        }
        st.mark(3);
        const int act = e_action(bestw0);
        u64 cown, copp, lg;
        CoopChild<G>::run(pown, popp, act, sub, &cown, &copp, &lg);  // lane-cooperative: -1.4 us per tree step (NOTEBOOK round 3)
        const u32 id = n_nodes_g++;
        const int tm = (depth & 1) ? root.tm : -root.tm;  // child's mover: the colours alternate down the walk (passes included)
        int tv = 0;
        const bool term = G::terminal(cown, copp, tm, lg, &tv);
        lp.own = cown; lp.opp = copp; lp.legal = term ? 0 : lg;
        lp.info = (term ? kTerm : 0u) | ((u32)(tv + 1) << 9) | ((tm == 1 ? 1u : 0u) << 11);
        const u32 w0 = bestw0 | ((term ? 1u : 0u) << kTermShift) | ((u32)(tv + 1) << kValShift);
        if (lead) {
            Node ch;
            ch.own = cown; ch.opp = copp; ch.legal = lp.legal; ch.edge0 = 0; ch.info = lp.info;
            nodes[id] = ch;
            edges[eidx].w0 = w0; edges[eidx].w3 = id;  // (the child's first edge / edge count follow with its expansion)
            c.v[CNT_ENV_STEPS]++; c.v[CNT_PATH_NODES]++;
        }
        if (depth < E.maxd) sink.put(depth, sub, eidx, w0, bestW);
        else if (lead) atomicOr(&E.flags[FLAG_ERR], ERR_DEPTH);
        depth++;
        leaf = id; kind = term ? LEAF_TERMINAL : LEAF_EVAL; tval = (float)tv;
        if (!kLeafPar && E.ecache && !term) {  // evaluated before in this search? (wave-uniform branch: a kernel argument; no cache with K > 1)
            u32 src = 0, src_e0 = 0;
            if (tt_lookup_insert<kGW>(E, g, sub, cown, copp, root.tt_gen, root.prev_nodes, id, src, src_e0)) { kind = LEAF_COPY; lp.src = src; lp.src_e0 = src_e0; }
        }
        st.mark(4);
        break;
    }
    depth_out = depth;
}

// k-th (0-based) set bit of m, or -1
__device__ __forceinline__ int nth_bit(u64 m, int k) {
    if (k >= popc64(m)) return -1;
    u32 w = (u32)m;
    int pos = 0, c = __popc(w);
    if (k >= c) { k -= c; w = (u32)(m >> 32); pos = 32; }
    c = __popc(w & 0xFFFFu); if (k >= c) { k -= c; w >>= 16; pos += 16; }
    c = __popc(w & 0xFFu);   if (k >= c) { k -= c; w >>= 8;  pos += 8; }
    c = __popc(w & 0xFu);    if (k >= c) { k -= c; w >>= 4;  pos += 4; }
    c = __popc(w & 0x3u);    if (k >= c) { k -= c; w >>= 2;  pos += 2; }
    return pos + (k >= (int)(w & 1u) ? 1 : 0);
}

// how dev_expand writes a fresh edge: the engine's packed record, or the private record of the tic-tac-toe
// fused search (plain N in word 0, its own child header in word 3)
struct EdgeFmtPacked { static __device__ __forceinline__ Edge make(float P, int a) { Edge e; e.w0 = (u32)a << kActShift; e.W = 0.0f; e.P = P; e.w3 = 0; return e; } };
struct EdgeFmtTttFused { static __device__ __forceinline__ Edge make(float P, int a) { Edge e; e.w0 = 0; e.W = 0.0f; e.P = P; e.w3 = (u32)a << 24; return e; } };

// M3: masked softmax over the legal actions (ascending), edges bump-allocated.  `legal` is the
// leaf's legal mask (known to the caller: the root's or the node select just created).
// `info` = the leaf's header word as created (child count 0): the header is rewritten, never re-read.
// Returns the number of edges written (they start at the old n_edges_g).
// kUniform: the caller's logits are all equal (the uniform evaluator, BASELINE cfg 2).  The spec's arithmetic then
// collapses without changing a bit: m = 0, every e = expf_spec(0) = 1.0 exactly, their sequential sum is the integer n
// exactly, P = 1 / float(n) by the same correctly rounded division -- no exponentials, no serial sum, no logits.
template <class G, int kGW = G::GW, bool kHeader = true, class Fmt = EdgeFmtPacked, bool kUniform = false>
__device__ __forceinline__ int dev_expand(const EngineDev& E, int g, int sub, u32 leaf, u64 legal, u32 info,
                                          const LogitSrc& ls, u32& n_edges_g, Cnt& c, Stamps& st) {
    constexpr int kCH = (G::MAXCH + kGW - 1) / kGW;
    Node* nd = E.nodes + (size_t)g * E.ncap + leaf;
    const u32 e0 = n_edges_g;
    Edge* ed = E.edges + (size_t)g * E.ecap + e0;
    const int room = E.ecap - (int)e0;
    int n = 0;
    if (legal == 0) {  // forced pass: one edge, P = 1
        if (room >= 1) {
            if (sub == 0) ed[0] = Fmt::make(1.0f, kPass);
            n = 1;
        }
    } else {
        n = popc64(legal);
        if (n > room) { if (sub == 0) atomicOr(&E.flags[FLAG_ERR], ERR_EDGE_OVERFLOW); n = room; }
        // this lane's moves: the sub-th, (sub+GW)-th, ... legal actions
        int a[kCH]; float x[kCH];
        float m = -__builtin_inff();
        u32 rest = (u32)legal;  // small boards (tic-tac-toe: 9 cells): walk the mask instead of a rank search per move
        if (G::NA <= 32)
            for (int j = 0; j < sub; ++j) rest &= rest - 1u;
#pragma unroll
        for (int k = 0; k < kCH; ++k) {
            if (G::NA <= 32) {  // this lane's k-th move = the lowest bit left; then skip the other lanes' kGW - 1 moves
                a[k] = (sub + kGW * k < n && rest) ? (int)__builtin_ctz(rest) : -1;
#pragma unroll
                for (int j = 0; j < kGW; ++j) rest &= rest - 1u;
            } else {
                a[k] = (sub + kGW * k < n) ? nth_bit(legal, sub + kGW * k) : -1;
            }
            if (!kUniform) {
                x[k] = a[k] >= 0 ? ls(a[k]) : -__builtin_inff();
                m = x[k] > m ? x[k] : m;
            }
        }
        if (!kUniform) m = group_max<kGW>(m);
        st.mark(1);  // (the evaluator's row has arrived)
        float ex[kCH];
#pragma unroll
        for (int k = 0; k < kCH; ++k) ex[k] = a[k] >= 0 ? (kUniform ? 1.0f : expf_spec(x[k] - m)) : 0.0f;
        // ascending-action serial sum (the spec's order): the partial sum travels up the group one lane per step
        // (lane t adds its own term to what lane t-1 holds), every step one DPP add; lanes past the last move hold
        // +0.0, which leaves a positive sum unchanged, so the chain runs its full length without tests.
        float s = kUniform ? (float)n : 0.0f;
#pragma unroll
        for (int k = 0; k < kCH; ++k) {
            if (!kUniform && kGW * k < n) {
                float part = s + ex[k];  // (lane 0's is the true partial sum; the others are overwritten below)
#pragma unroll
                for (int t = 1; t < kGW; ++t) {
                    const float cand = row_shr1(part) + ex[k];
                    part = sub == t ? cand : part;
                }
                s = __shfl(part, kGW - 1, kGW);
            }
        }
        if (sub == 0 && !(s >= 1.0f && s <= 3.0e38f)) atomicOr(&E.flags[FLAG_ERR], ERR_EVAL_NONFINITE);  // (the maximum's term is exactly 1)
        float pr[kCH];
#pragma unroll
        for (int k = 0; k < kCH; ++k) pr[k] = a[k] >= 0 ? fdiv(ex[k], s) : 0.0f;
#pragma unroll
        for (int k = 0; k < kCH; ++k)
            if (a[k] >= 0) ed[sub + kGW * k] = Fmt::make(pr[k], a[k]);
    }
    if (sub == 0) {
        if (kHeader) *reinterpret_cast<uint2*>(&nd->edge0) = make_uint2(e0, (info & ~0xFFu) | (u32)n);  // edge0, info: one 8-byte store
        c.v[CNT_EXPANDED]++;
        c.v[CNT_CHILD_WRITTEN] += (u32)n;
    }
    n_edges_g = e0 + (u32)n;
    return n;
}

// M3 for a leaf whose position was evaluated earlier in this search (evaluation cache): the same edges -- actions in
// ascending order, the priors the masked softmax gave the first time, bit for bit -- copied from that node's block;
// N = 0, W = 0, no child.  legal / info as for dev_expand.  Returns the number of edges written.
template <class G, int kGW = G::GW>
__device__ __forceinline__ int dev_expand_copy(const EngineDev& E, int g, int sub, u32 leaf, u64 legal, u32 info, u32 src_e0,
                                               bool from_prev, u32& n_edges_g, Cnt& c) {
    constexpr int kCH = (G::MAXCH + kGW - 1) / kGW;
    Node* nd = E.nodes + (size_t)g * E.ncap + leaf;
    const u32 e0 = n_edges_g;
    Edge* ed = E.edges + (size_t)g * E.ecap + e0;
    const Edge* from = (from_prev ? E.edges_alt : E.edges) + (size_t)g * E.ecap + src_e0;
    const int room = E.ecap - (int)e0;
    int n = legal == 0 ? 1 : popc64(legal);
    if (n > room) { if (sub == 0) atomicOr(&E.flags[FLAG_ERR], ERR_EDGE_OVERFLOW); n = room; }
    Edge got[kCH];
#pragma unroll
    for (int k = 0; k < kCH; ++k) if (sub + kGW * k < n) got[k] = from[sub + kGW * k];
#pragma unroll
    for (int k = 0; k < kCH; ++k) if (sub + kGW * k < n) ed[sub + kGW * k] = EdgeFmtPacked::make(got[k].P, e_action(got[k].w0));
    if (sub == 0) {
        *reinterpret_cast<uint2*>(&nd->edge0) = make_uint2(e0, (info & ~0xFFu) | (u32)n);
        c.v[CNT_EXPANDED]++;
        c.v[CNT_CHILD_WRITTEN] += (u32)n;
        c.v[CNT_CACHE_HITS]++;
        if (from_prev) c.v[CNT_CACHE_HITS_PREV]++;
    }
    n_edges_g = e0 + (u32)n;
    return n;
}

// M4: W is stored for the mover at the parent, so the sign flips every ply; one path edge per lane.
// N and W of every path edge were captured by the select walk (nothing else touches this game's tree
// in between), so the backup is one 8-byte store per path edge and reads nothing but the path.  The
// deepest edge leads to the leaf: when the leaf was expanded just now (exp_n > 0 edges from exp_e0),
// its edge count / first edge go into that edge's words with the same stores.
template <class PE>
__device__ __forceinline__ uint2 backup_edge(Edge* edges, const PE& pe, float val, bool deepest, u32 leaf, u32 exp_e0, int exp_n) {
    u32 w0 = pe.w0 + 1u;
    if (deepest && exp_n > 0) {
        w0 |= (u32)exp_n << kNchShift;
        edges[pe.eidx].w3 = leaf | (exp_e0 << kChildBits);
    }
    const uint2 wr = make_uint2(w0, __float_as_uint(pe.W + val));
    *reinterpret_cast<uint2*>(edges + pe.eidx) = wr;
    return wr;
}

template <int kGW, class PE>
__device__ __forceinline__ void dev_backup(const EngineDev& E, int g, int sub, int depth, float v, const PE* path,
                                           u32 leaf, u32 exp_e0, int exp_n, Cnt& c) {
    Edge* edges = E.edges + (size_t)g * E.ecap;
    const int dmax = depth < E.maxd ? depth : E.maxd;
    for (int d = sub; d < dmax; d += kGW) {
        const PE pe = path[d];
        const float val = ((dmax - 1 - d) & 1) ? v : -v;  // deepest edge gets -v
        backup_edge(edges, pe, val, d == depth - 1, leaf, exp_e0, exp_n);
    }
    if (sub == 0) c.v[CNT_EDGES_BACKED] += (u32)dmax;
}

// The proof pass behind the backup of a walk that ended in a terminal or proven leaf: upwards from the deepest
// path edge, the node rule over the block of edges the path edge lies in -- lanes over edges, one OR across the group.  A decided
// parent marks the path edge into it (behind the backup's own store of that edge) and the pass goes on one level up; it stops
// at the first undecided parent and at the root, whose value goes to the solver buffer.  Path entries hold no w3: the block of
// path edge d is the root's (edge 0, root_n) or comes from the words of path edge d - 1.  A truncated path (depth > maxd, ERR_DEPTH)
// proves nothing.  re0: the caller's register copy of root edge `sub`.
template <class G>
__device__ __forceinline__ void dev_prove(const EngineDev& E, const SolveDev& Sv, int g, int sub, const PathEnt* path, int depth,
                                          int root_n, Edge& re0) {
    constexpr int kGW = G::GW;
    if (depth < 1 || depth > E.maxd) return;
    Edge* edges = E.edges + (size_t)g * E.ecap;
    const int root_rec = Sv.root[g];
    u32 n_new = 0;
    int d = depth - 1;
    PathEnt pe = path[d];
    const bool at_proven = !e_term(pe.w0);  // the walk stopped at a proven edge that is not terminal
    for (;;) {
        group_fence();  // the backup's stores and the mark below are read here
        u32 b0 = 0; int n = root_n;
        PathEnt up = pe;
        if (d > 0) { up = path[d - 1]; b0 = e_edge0(edges[up.eidx].w3); n = e_nch(up.w0); }
        if (b0 + (u32)n > (u32)E.ecap) break;  // (never: the walk scored these edges)
        u32 bits = 0;
        for (int i = sub; i < n; i += kGW) bits |= solver_edge_bits(e_cval(edges[b0 + i].w0));
        bits = group_or_u32<kGW>(bits);
        const int pv = solver_node_value(bits, n);
        if (pv == kSolverUndecided) break;
        if (d == 0) {  // the root
            if (root_rec == 0) { n_new++; if (sub == 0) Sv.root[g] = pv + 2; }
            break;
        }
        n_new++;
        const u32 w0n = ((up.w0 + 1u) & ~(3u << kValShift)) | ((u32)(pv + 1) << kValShift) | kProven;  // (up.w0 + 1: what the backup stored)
        if (sub == 0) edges[up.eidx].w0 = w0n;
        if (d == 1 && (u32)sub == up.eidx) re0.w0 = w0n;
        --d; pe = up;
    }
    if (sub == 0) {
        if (n_new) atomicAdd(&Sv.counts[0], n_new);
        if (at_proven) atomicAdd(&Sv.counts[1], 1u);
    }
}

template <class G>
__device__ __forceinline__ bool dev_root_init(const EngineDev& E, int g) {
    u64 own = E.g_own[g], opp = E.g_opp[g];
    int tm = E.g_to_move[g];
    u64 lg = G::legal(own, opp);
    int tv;
    if (G::terminal(own, opp, tm, lg, &tv)) {
        atomicOr(&E.flags[FLAG_ERR], ERR_TERMINAL_ROOT);
        return false;
    }
    Node r; r.own = own; r.opp = opp; r.legal = lg; r.edge0 = 0; r.info = (tm == 1 ? 1u : 0u) << 11;
    E.nodes[(size_t)g * E.ncap] = r;
    E.hot[g].leaf_legal = lg; E.hot[g].leaf_info = r.info;  // what the expansion of this "leaf" reads
    return true;
}

// start position (+ fixed two-ply openings) of the game with global id gid
template <class G>
__device__ __forceinline__ void dev_start_game(const EngineDev& E, int g, int round) {
    u64 own, opp;
    G::start(&own, &opp);
    int tm = 1, made = 0;
    if (G::kGame == 1 && E.openings) {  // the 12 two-ply openings are an 8x8 notion
        u64 gid = E.id_base + (u64)round * E.id_stride + (u64)g;
        int k = (int)(gid % 12ULL);
        int pick[2] = {k / 3, k % 3};
        for (int i = 0; i < 2; ++i) {
            u64 l = G::legal(own, opp);
            for (int j = 0; j < pick[i]; ++j) l &= l - 1;
            u64 c0, c1;
            G::apply(own, opp, ctz64(l), &c0, &c1);
            own = c0; opp = c1; tm = -tm; made++;
        }
    }
    E.g_own[g] = own; E.g_opp[g] = opp; E.g_to_move[g] = (int8_t)tm;
    E.g_moves[g] = made; E.g_nex[g] = 0; E.g_round[g] = round; E.g_passes[g] = 0; E.g_state[g] = 0;
    if (E.reuse) E.g_reuse[g] = 0;
    E.hot[g].root_base = 0;
}

template <class G>
__global__ void __launch_bounds__(256) k_reset_games(EngineDev E) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B) return;
    dev_start_game<G>(E, g, 0);
    if (E.stagger > 0) {  // bench only: pre-advance by (g % stagger) pseudo-random legal plies
        u64 own = E.g_own[g], opp = E.g_opp[g];
        int tm = E.g_to_move[g], made = E.g_moves[g], want = g % E.stagger;
        bool ok = true;
        for (int k = 0; k < want && ok; ++k) {
            u64 lg = G::legal(own, opp);
            int tv;
            if (G::terminal(own, opp, tm, lg, &tv)) { ok = false; break; }
            if (lg == 0) { u64 t = own; own = opp; opp = t; tm = -tm; continue; }
            int pick = (int)(rng_draw(E.seed ^ 0x5AFEC0DEULL, (u64)g, (u64)k) % (u64)popc64(lg));
            for (int j = 0; j < pick; ++j) lg &= lg - 1;
            u64 c0, c1;
            G::apply(own, opp, ctz64(lg), &c0, &c1);
            own = c0; opp = c1; tm = -tm; made++;
        }
        u64 lg = G::legal(own, opp);
        int tv;
        if (ok && !G::terminal(own, opp, tm, lg, &tv)) {
            if (lg == 0) { u64 t = own; own = opp; opp = t; tm = -tm; }
            E.g_own[g] = own; E.g_opp[g] = opp; E.g_to_move[g] = (int8_t)tm; E.g_moves[g] = made;
        }
    }
    for (int r = 0; r < E.rounds; ++r) { E.ex_len[(size_t)r * E.B + g] = -1; E.ex_winner[(size_t)r * E.B + g] = 0; }
    if (g == 0) { E.flags[FLAG_ERR] = 0; E.flags[FLAG_FINISHED] = 0; E.flags[FLAG_NEVAL] = 0; E.flags[FLAG_NEVAL + 1] = 0; }
}

__global__ void __launch_bounds__(256) k_set_roots(EngineDev E, const u64* own, const u64* opp, const int8_t* tm) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B) return;
    E.g_own[g] = own[g]; E.g_opp[g] = opp[g]; E.g_to_move[g] = tm[g];
    E.g_state[g] = tm[g] == 0 ? 1 : 0;  // to_move 0 = slot not in use (the arena searches a subset of its games)
    if (E.reuse) E.g_reuse[g] = 0;
    E.hot[g].root_base = 0;
    E.g_moves[g] = 0; E.g_nex[g] = 0; E.g_round[g] = 0; E.g_passes[g] = 0;
    if (g == 0) { E.flags[FLAG_ERR] = 0; E.flags[FLAG_FINISHED] = 0; E.flags[FLAG_NEVAL] = 0; E.flags[FLAG_NEVAL + 1] = 0; }
}

// Subtree reuse: copy the subtree below node `src_root` of the previous move's arena to the front of
// this move's arena, breadth first (Cheney): node 0 = the new root, a node's edges stay one contiguous block in
// ascending action order, child ids and edge0 are rewritten.  One lane per game; a few hundred nodes per move.
// (With noise on, k_root_noise then makes a fresh Dirichlet draw on the kept root's stored priors, as for a new root.)
template <class G>
__device__ __forceinline__ void dev_reroot(const EngineDev& E, int g, u32 src_root) {
    const Node* sn = E.nodes_alt + (size_t)g * E.ncap;
    const Edge* se = E.edges_alt + (size_t)g * E.ecap;
    Node* dn = E.nodes + (size_t)g * E.ncap;
    Edge* de = E.edges + (size_t)g * E.ecap;
    u32 n_dst = 1, e_dst = 0;
    dn[0] = sn[src_root];
    // nodes are laid out in breadth-first order and so are their edge blocks: the first edge of the node that gets
    // id k is the number of edges of all nodes before it, known the moment k is handed out
    u32 e_next = dn[0].info & 0xFFu;
    E.hot[g].root_n = e_next;
    for (u32 i = 0; i < n_dst; ++i) {
        Node nd = dn[i];  // edge0 still points into the source arena
        if (nd.info & kTerm) continue;
        const u32 n = nd.info & 0xFFu, s0 = nd.edge0;
        for (u32 j = 0; j < n; ++j) {
            Edge e = se[s0 + j];
            const u32 child = e_child(e.w3);
            if (child) {
                const u32 id = n_dst++;
                const Node cn = sn[child];
                dn[id] = cn;
                e.w3 = id | (e_next << kChildBits);
                e_next += cn.info & 0xFFu;  // (0 for terminal / not yet expanded nodes)
            }
            de[e_dst + j] = e;
        }
        dn[i].edge0 = e_dst;
        e_dst += n;
    }
    E.hot[g].n_nodes = n_dst; E.hot[g].n_edges = e_dst;
}

template <class G>
__global__ void __launch_bounds__(256) k_root_begin(EngineDev E, u32 tt_gen, int carry_ok) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B) return;
    uint8_t kind = LEAF_NONE;
    if (E.ecache) {  // entries older than the previous search are free slots from now on
        const u32 gen_prev = tt_gen == 1u ? kTtGenMax - 1u : tt_gen - 1u;
        // carry-over: the other arena holds this slot's previous tree only if the slot took part in the previous search
        const bool carry = E.ecache == 2 && carry_ok && E.hot[g].last_gen == gen_prev;
        E.hot[g].prev_nodes = carry ? E.hot[g].n_nodes : 0u;
        E.hot[g].tt_gen = tt_gen;
        if (E.g_state[g] == 0) E.hot[g].last_gen = tt_gen;
    }
    const u32 keep = (E.reuse && E.g_state[g] == 0) ? E.g_reuse[g] : 0u;
    if (keep) {
        dev_reroot<G>(E, g, keep);
        kind = LEAF_READY;
        E.hot[g].leaf_node = 0; E.hot[g].depth = 0;
    } else if (E.g_state[g] == 0 && dev_root_init<G>(E, g)) {
        kind = LEAF_EVAL;
        E.hot[g].n_nodes = 1; E.hot[g].n_edges = 0; E.hot[g].leaf_node = 0; E.hot[g].depth = 0;
        E.hot[g].root_base = 0;
    }
    const size_t r0 = (size_t)g * E.K;  // leaf rows g*K + j (K = 1: row g)
    E.leaf_own[r0] = E.g_own[g]; E.leaf_opp[r0] = E.g_opp[g];
    E.leaf_kind[r0] = kind;
    u32 slot = 0;
    if (E.compact && kind == LEAF_EVAL) {
        slot = atomicAdd(&E.flags[FLAG_NEVAL + 1], 1u);
        E.hot[g].leaf_slot = slot; E.c_own[slot] = E.g_own[g]; E.c_opp[slot] = E.g_opp[g];
    }
    if (E.K > 1) {  // leaf-parallel: the root is walk 0's leaf, the other walks have none
        LeafRec r; r.legal = E.hot[g].leaf_legal; r.node = 0; r.info = E.hot[g].leaf_info; r.slot = slot; r.depth = 0;
        r.kind = kind; r.v = 0.0f;
        E.lrec[r0] = r;
        for (int j = 1; j < E.K; ++j) { E.lrec[r0 + j].kind = LEAF_NONE; E.leaf_kind[r0 + j] = LEAF_NONE; }
    }
    if (g == 0) E.flags[FLAG_NEVAL] = 0;
}

// Dirichlet root noise, its own small kernel so that the sampler's registers stay out of the tree
// kernels (inlined into the expansion it took k_tree_step from 78 to 129 VGPRs and the cfg-2 kernel from 93 to 219):
// P' = (1 - eps) P + eps g / sum(g) over the root's edges in ascending action order, for every active game whose
// root is expanded -- freshly (by the expand-only tree step before this launch) or kept from the previous move.
// kCap: the masked form (playout cap randomisation) -- noise on the roots of the FULL searches only, same key,
// same bits; with kCap = false it is k_root_noise's code exactly.
template <bool kCap>
__device__ __forceinline__ void root_noise_body(const EngineDev& E, const u32* budget) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B || E.g_state[g] != 0) return;
    if (kCap && budget[g] < (u32)E.sims) return;
    const Node r = E.nodes[(size_t)g * E.ncap];
    const int n = (int)(r.info & 0xFFu);
    if (n == 0 || r.legal == 0) return;  // not expanded / a forced-pass root (P = 1 stays)
    Edge* ed = E.edges + (size_t)g * E.ecap + r.edge0;
    const u64 gid = E.id_base + (u64)E.g_round[g] * E.id_stride + (u64)g, ply = (u64)E.g_moves[g];
    float gs = 0.0f;
    for (int i = 0; i < n; ++i) gs = gs + gamma_spec(E.dir_alpha, E.seed, gid, ply, i);
    if (!(gs > 0.0f)) return;
    const float keep = 1.0f - E.dir_eps;
    for (int i = 0; i < n; ++i) {
        float t1 = keep * ed[i].P;
        float t2 = E.dir_eps * fdiv(gamma_spec(E.dir_alpha, E.seed, gid, ply, i), gs);
        ed[i].P = t1 + t2;
    }
}
__global__ void __launch_bounds__(64) k_root_noise(EngineDev E) { root_noise_body<false>(E, nullptr); }
__global__ void __launch_bounds__(64) k_cap_noise(EngineDev E, CapDev Cp) { root_noise_body<true>(E, Cp.budget); }

// every slot's budget for the search k_root_begin has just set up: sims with probability full_q / 65536, else
// fast, drawn from (seed ^ kCapKey, game id, moves made) -- the key of the Dirichlet noise; 0 for a slot that is not in a game
__global__ void __launch_bounds__(256) k_cap_budget(EngineDev E, CapDev Cp) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B) return;
    u32 b = 0;
    if (E.g_state[g] == 0) {
        const u64 gid = E.id_base + (u64)E.g_round[g] * E.id_stride + (u64)g;
        b = cap_budget(E.seed, gid, (u64)E.g_moves[g], E.sims, Cp.fast, Cp.full_q);
    }
    Cp.budget[g] = b;
}

// synthetic evaluators as a separate step (used by the step-by-step API)
// (over the K*B leaf rows: grid-stride, the grid covers B)
template <class G>
__global__ void __launch_bounds__(256) k_eval_synth(EngineDev E, int eval_kind) {
    const int rows = E.B * E.K;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < rows; g += gridDim.x * blockDim.x) {
        if (E.leaf_kind[g] != LEAF_EVAL) continue;
        u64 h = hash_pos(E.leaf_own[g], E.leaf_opp[g]);
        float* row = E.logits + (size_t)g * G::NA;
        for (int a = 0; a < G::NA; ++a) row[a] = eval_kind == BZ_EVAL_HASH ? hash_logit(h, a) : 0.0f;
        E.value[g] = eval_kind == BZ_EVAL_HASH ? hash_value(h) : 0.0f;
    }
}

// One tree step for every game (16 lanes per game): [expand + backup of the previous leaf] and/or
// [select of the next leaf].  With a net in the loop a simulation is exactly two launches:
// this kernel and the net.  The kernel is a dependent-access chain per game (every game of the launch is
// in flight at once), so its time is the number of memory round trips on the longest chain: one for all
// per-game words and the path (independent loads), one for the evaluator's row, then one per level of the walk.
// keeps a loaded value "used" at this point of the program: the loads above it cannot be sunk into the branches
// that consume them, so they go out back to back and complete in ONE memory round trip
template <class T> __device__ __forceinline__ void pin(T& x) { asm volatile("" : "+v"(x)); }

// The body of every per-step kernel but k_leaf_step, under the search mode M (Mode, above): with M = 0 it is k_tree_step's code
// exactly, and every bit adds only what its rule needs.
template <class G, unsigned M>
__device__ __forceinline__ void tree_step_body(const EngineDev& E, const ModeArgs& A, int do_expand, int do_select, u32 sim_idx) {
    constexpr bool kGumbel = Mode<M>::gumbel, kCap = Mode<M>::cap, kForced = Mode<M>::forced, kFpu = Mode<M>::fpu, kGfull = Mode<M>::gfull,
                   kSolve = Mode<M>::solve, kStop = Mode<M>::stop, kPace = Mode<M>::pace;
    static_assert(!Mode<M>::leaf, "search mode: the leaf-parallel step is k_leaf_step's own body");
    constexpr int kGW = G::GW;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int g = t / kGW, sub = t % kGW;
    Cnt c = {};
    Stamps st; st.start();
    // packed-leaf slots: ONE atomic on the shared counter per workgroup.  Same-address atomics are served one after the
    // other (~10 ns each): one per wave -- 1024 per launch at 4096 games -- was half of this kernel's time.
    __shared__ u32 s_need, s_base;
    if (threadIdx.x == 0) s_need = 0;
    __syncthreads();
    bool want_slot = false; u32 my_rank = 0; u64 slot_own = 0, slot_opp = 0;
    if (g < E.B) {
        PathEnt* path = E.path + (size_t)g * E.maxd;
        // ---- round trip 1: every per-game word this step can need + the first kGW path entries, all independent
        int kind = E.leaf_kind[g], state = E.g_state[g];
        const GameHot hot = E.hot[g];
        u32 leaf = hot.leaf_node, ninfo = hot.leaf_info, ne = hot.n_edges, nn = hot.n_nodes, row = E.compact ? hot.leaf_slot : (u32)g;
        int depth0 = (int)hot.depth, root_n = (int)hot.root_n, rtm = E.g_to_move[g];
        u64 nlegal = hot.leaf_legal, rown = E.g_own[g], ropp = E.g_opp[g];
        u32 root_base = E.reuse ? hot.root_base : 0u;
        PathEnt pe0 = path[sub];  // (maxd >= kGW for every game)
        u32 bud = 0;
        if (kCap) { bud = A.budget[g]; pin(bud); }
        [[maybe_unused]] float rw;
        if constexpr (kFpu) { rw = A.fp->root_w[g]; pin(rw); }
        [[maybe_unused]] int made = 0;
        if constexpr (kStop) { made = E.g_moves[g]; pin(made); }
        // the walk's first load too: root edges 0..kGW-1 (the root's edges start at index 0; whatever this step's
        // backup / expansion changes in them is patched in registers below) -- their latency hides behind the
        // evaluator row's round trip and the softmax instead of heading the walk
        Edge* const edges_g = E.edges + (size_t)g * E.ecap;
        Edge re0 = edges_g[sub];
        pin(re0.w0); pin(re0.W); pin(re0.P); pin(re0.w3);
        bool pre_ok = true;
        pin(kind); pin(state); pin(leaf); pin(ninfo); pin(ne); pin(nn); pin(row); pin(depth0); pin(root_n); pin(rtm);
        pin(nlegal); pin(rown); pin(ropp); pin(root_base); pin(pe0.eidx); pin(pe0.w0); pin(pe0.W);
        const bool active = state == 0 && kind != LEAF_NONE;
        // a slot at its budget expands and backs up its last leaf below, selects nothing and is left LEAF_NONE: idle from then on
        bool walk = kCap ? (active && sim_idx < bud) : active;
        [[maybe_unused]] u32 my_sim = sim_idx;  // kPace: the slot's own simulation number
        [[maybe_unused]] bool seeded_root = false;
        if constexpr (kPace) {  // a launch the slot skipped left it LEAF_NONE: whether it walks is the schedule's word, not the leaf's
            const u32 sd = hot.seeded, r = sd == kPaceIdle ? 0u : (u32)E.sims - sd;
            walk = state == 0 && pace_walks(sim_idx, r, (u32)E.sims);
            my_sim = sd + pace_done(sim_idx, r, (u32)E.sims);
            seeded_root = sd != 0u && leaf == 0u;
        }
        st.mark(0);
        if (do_expand && (kind == LEAF_EVAL || kind == LEAF_TERMINAL || kind == LEAF_COPY)) {
            float v;
            u32 e0 = ne; int n = 0;
            if (kPace && kind == LEAF_EVAL && seeded_root) {  // the seed expanded this root: its row is counted, its tree stays
                v = E.value[row];
                if (sub == 0) {
                    if (!(v >= -3.0e38f && v <= 3.0e38f)) atomicOr(&E.flags[FLAG_ERR], ERR_EVAL_NONFINITE);
                    c.v[CNT_NET_LEAVES]++;
                }
            } else if (kind == LEAF_EVAL) {  // ---- round trip 2: the evaluator's row
                LogitSrc ls; ls.kind = BZ_EVAL_EXTERNAL; ls.h = 0; ls.row = E.logits + (size_t)row * G::NA;
                v = E.value[row];
                if (sub == 0 && !(v >= -3.0e38f && v <= 3.0e38f)) atomicOr(&E.flags[FLAG_ERR], ERR_EVAL_NONFINITE);
                n = dev_expand<G>(E, g, sub, leaf, nlegal, ninfo, ls, ne, c, st);
                if (sub == 0) {
                    E.hot[g].n_edges = ne; c.v[CNT_NET_LEAVES]++; if (leaf == 0) E.hot[g].root_n = (u32)n;
                    if (E.ecache) E.node_v[(size_t)g * E.ncap + leaf] = v;  // what a later repeat of this position copies
                    if (kGumbel && leaf == 0) A.gm->vroot[g] = v;
                    if constexpr (kGfull) A.gi->node_v[(size_t)g * E.ncap + leaf] = v;
                }
                if (leaf == 0) { root_n = n; pre_ok = false; }  // the root's edges did not exist when re0 was fetched
            } else if (kind == LEAF_COPY) {  // ---- round trip 2: the first evaluation's edges and value (evaluation cache)
                const bool from_prev = (hot.copy_src & kSrcPrev) != 0u;
                v = (from_prev ? E.node_v_alt : E.node_v)[(size_t)g * E.ncap + (hot.copy_src & ~kSrcPrev)];
                n = dev_expand_copy<G>(E, g, sub, leaf, nlegal, ninfo, hot.copy_e0, from_prev, ne, c);
                if (sub == 0) {
                    E.hot[g].n_edges = ne; E.node_v[(size_t)g * E.ncap + leaf] = v;
                    if (kGumbel && leaf == 0) A.gm->vroot[g] = v;
                    if constexpr (kGfull) A.gi->node_v[(size_t)g * E.ncap + leaf] = v;
                }
            } else {
                v = (float)((int)((ninfo >> 9) & 3u) - 1);
            }
            // backup: path entries 0..kGW-1 are in registers already; deeper walks (rare) load theirs
            Edge* edges = edges_g;
            const int dmax = depth0 < E.maxd ? depth0 : E.maxd;
            uint2 wr = make_uint2(0u, 0u);
            if (sub < dmax) wr = backup_edge(edges, pe0, ((dmax - 1 - sub) & 1) ? v : -v, sub == depth0 - 1, leaf, e0, n);
            for (int d = sub + kGW; d < dmax; d += kGW)
                backup_edge(edges, path[d], ((dmax - 1 - d) & 1) ? v : -v, d == depth0 - 1, leaf, e0, n);
            if (sub == 0) c.v[CNT_EDGES_BACKED] += (u32)dmax;
            if constexpr (kFpu) if (dmax >= 1) {  // Wr = Wr + what path entry 0 just added to its edge's W, one addition per simulation
                rw = (sim_idx == 1u ? 0.0f : rw) + (((dmax - 1) & 1) ? v : -v);
                if (sub == 0) A.fp->root_w[g] = rw;
            }
            if (dmax >= 1) {  // the path's root edge (lane 0 wrote it): the same words into the lane that holds it in re0
                const u32 pe_e = (u32)__shfl((int)pe0.eidx, 0, kGW), w0n = (u32)__shfl((int)wr.x, 0, kGW), Wn = (u32)__shfl((int)wr.y, 0, kGW);
                if ((u32)sub == pe_e) {
                    re0.w0 = w0n; re0.W = __uint_as_float(Wn);
                    if (depth0 == 1 && n > 0) re0.w3 = leaf | (e0 << kChildBits);
                }
            }
            if constexpr (kSolve) if (kind == LEAF_TERMINAL) dev_prove<G>(E, *A.sv, g, sub, path, depth0, root_n, re0);
        }
        if constexpr (kStop) {  //  sim_idx simulations are backed up: is the move decided?  (a branch per game)
            const u32 left = (u32)E.sims - sim_idx;
            if (do_select && walk && pre_ok && made >= E.temp_moves && early_stop_possible(root_n, sim_idx, left)) {
                constexpr int kCH = (G::MAXCH + kGW - 1) / kGW;
                group_fence();  // the root edge the backup above wrote is read below when it lies beyond re0
                u32 Nk[kCH], key = 0;
#pragma unroll
                for (int k = 0; k < kCH; ++k) {
                    const int i = k * kGW + sub;
                    Nk[k] = 0;
                    if (i < root_n) {
                        Nk[k] = e_N(k == 0 ? re0.w0 : edges_g[i].w0);
                        const u32 ky = early_stop_key(Nk[k], i);
                        key = ky > key ? ky : key;
                    }
                }
                key = group_max_u32<kGW>(key);
                const u32 NL = early_stop_leader_N(key);
                const int L = early_stop_leader(key);
                u32 open = 0;
#pragma unroll
                for (int k = 0; k < kCH; ++k) {
                    const int i = k * kGW + sub;
                    if (i < root_n && early_stop_catches(Nk[k], i, NL, L, left)) open = 1u;
                }
                open = group_or_u32<kGW>(open);
                if (!open) {
                    walk = false;
                    if (sub == 0) A.sp->stop_at[g] = sim_idx;
                }
            }
            if (do_select && walk && sub == 0) A.sp->walked[0] = sim_idx + 1u;  // (every writer of a step stores the same word)
        }
        st.mark(2);
        if (do_select) {
            uint8_t kind8 = LEAF_NONE;
            if (walk) {
                group_fence();  // edges written above are read below
                u32 leaf2; int k2, depth; float tv;
                LeafPos lpos; lpos.own = 0; lpos.opp = 0; lpos.legal = 0; lpos.info = 0; lpos.src = 0; lpos.src_e0 = 0;
                RootRef root; root.own = rown; root.opp = ropp; root.tm = rtm; root.n = root_n;
                root.sumN = (kPace ? my_sim : sim_idx) + root_base; root.has_pre = pre_ok; root.pre = re0; root.tt_gen = hot.tt_gen; root.prev_nodes = hot.prev_nodes;
                PathHbm<kGW> sink; sink.p = path; sink.mine.eidx = 0; sink.mine.w0 = 0; sink.mine.W = 0.0f; sink.mine.pad = 0;
                const float fslot = (kForced && (!kCap || bud >= (u32)E.sims)) ? A.fo->k : 0.0f;
                dev_select<G, M>(E, g, sub, root, nn, leaf2, k2, depth, tv, c, sink, lpos, st, A, fslot, kFpu ? rw : 0.0f);  // ---- one round trip per level
                sink.flush(sub, depth);
                if (sub == 0) {
                    E.hot[g].n_nodes = nn; E.hot[g].leaf_node = leaf2; E.hot[g].depth = (u32)depth;
                    if (k2 == LEAF_EVAL) {  // only an evaluated leaf's position is consumed (evaluator input)
                        E.leaf_own[g] = lpos.own; E.leaf_opp[g] = lpos.opp; E.hot[g].leaf_legal = lpos.legal; E.hot[g].leaf_info = lpos.info;
                        if (E.compact) { want_slot = true; my_rank = atomicAdd(&s_need, 1u); slot_own = lpos.own; slot_opp = lpos.opp; }
                    } else if (k2 == LEAF_COPY) {  // its evaluation exists already: no evaluator row, the next step copies it
                        E.hot[g].leaf_legal = lpos.legal; E.hot[g].leaf_info = lpos.info;
                        E.hot[g].copy_src = lpos.src; E.hot[g].copy_e0 = lpos.src_e0;
                    } else {  // terminal leaf (new or revisited): the backup needs its value only
                        E.hot[g].leaf_info = (u32)((int)tv + 1) << 9;
                    }
                }
                kind8 = (uint8_t)k2;
            }
            if (sub == 0) E.leaf_kind[g] = kind8;
            if (t == 0) E.flags[FLAG_NEVAL + ((sim_idx + 1u) & 1u)] = 0;  // the buffer the NEXT select packs into
        } else if (t == 0) {  // expand-only step (end of a search / step API): nothing is packed any more
            E.flags[FLAG_NEVAL] = 0; E.flags[FLAG_NEVAL + 1] = 0;
        }
    }
    if (do_select && E.compact) {  // (kernel arguments: the whole grid takes this branch or none of it)
        __syncthreads();
        if (threadIdx.x == 0) s_base = s_need ? atomicAdd(&E.flags[FLAG_NEVAL + (sim_idx & 1u)], s_need) : 0u;
        __syncthreads();
        if (want_slot) {
            const u32 slot = s_base + my_rank;
            E.hot[g].leaf_slot = slot; E.c_own[slot] = slot_own; E.c_opp[slot] = slot_opp;
        }
    }
    st.mark(5);
    cnt_flush<G::GW>(E, c);
    st.mark(6);
    st.flush(E.counters);
}

// The per-step kernels: each fills ModeArgs from its own kernel arguments (the mode's *Dev structs travel as kernel arguments, so
// EngineDev and every other kernel's code stay what they are) and runs tree_step_body under its mode.
template <class G>
__global__ void __launch_bounds__(256) k_tree_step(EngineDev E, int do_expand, int do_select, u32 sim_idx) {
    tree_step_body<G, 0u>(E, ModeArgs{}, do_expand, do_select, sim_idx);
}

// The tree step of a paced search ("The replay seed"): k_tree_step, every slot walking in its own launches.
template <class G>
__global__ void __launch_bounds__(256) k_pace_step(EngineDev E, int do_expand, int do_select, u32 sim_idx) {
    tree_step_body<G, kModePace>(E, ModeArgs{}, do_expand, do_select, sim_idx);
}

// The tree step of a Gumbel search: k_tree_step with the Gumbel root rule.  The root's statistics are read
// afresh after this step's backup (the group fence before the walk) by a serial loop over its edges.
template <class G>
__global__ void __launch_bounds__(256) k_gumbel_step(EngineDev E, GumbelDev Gm, int do_expand, int do_select, u32 sim_idx) {
    ModeArgs A; A.gm = &Gm;
    tree_step_body<G, kModeGumbel>(E, A, do_expand, do_select, sim_idx);
}

// ... with the Gumbel interior rule at every level below the root, and v_X stored with every expansion.
template <class G>
__global__ void __launch_bounds__(256) k_gfull_step(EngineDev E, GumbelDev Gm, GumbelInDev Gi, int do_expand, int do_select, u32 sim_idx) {
    ModeArgs A; A.gm = &Gm; A.gi = &Gi;
    tree_step_body<G, kModeGumbel | kModeGfull>(E, A, do_expand, do_select, sim_idx);
}

// The tree step under playout cap randomisation: k_tree_step, every slot walking for its own budget.
template <class G>
__global__ void __launch_bounds__(256) k_cap_step(EngineDev E, CapDev Cp, int do_expand, int do_select, u32 sim_idx) {
    ModeArgs A; A.budget = Cp.budget;
    tree_step_body<G, kModeCap>(E, A, do_expand, do_select, sim_idx);
}

// The tree step with forced playouts: k_tree_step / k_cap_step with the forced rule in the root's scores.
template <class G>
__global__ void __launch_bounds__(256) k_forced_step(EngineDev E, ForcedDev F, int do_expand, int do_select, u32 sim_idx) {
    ModeArgs A; A.fo = &F;
    tree_step_body<G, kModeForced>(E, A, do_expand, do_select, sim_idx);
}
template <class G>
__global__ void __launch_bounds__(256) k_forced_cap_step(EngineDev E, CapDev Cp, ForcedDev F, int do_expand, int do_select, u32 sim_idx) {
    ModeArgs A; A.budget = Cp.budget; A.fo = &F;
    tree_step_body<G, kModeForced | kModeCap>(E, A, do_expand, do_select, sim_idx);
}

// The tree steps with first-play urgency reduction: k_tree_step / k_cap_step / k_forced_step / k_forced_cap_step
// with the FPU rule at every level of the walk.
template <class G>
__global__ void __launch_bounds__(256) k_fpu_step(EngineDev E, FpuDev Fp, int do_expand, int do_select, u32 sim_idx) {
    ModeArgs A; A.fp = &Fp;
    tree_step_body<G, kModeFpu>(E, A, do_expand, do_select, sim_idx);
}
template <class G>
__global__ void __launch_bounds__(256) k_fpu_cap_step(EngineDev E, CapDev Cp, FpuDev Fp, int do_expand, int do_select, u32 sim_idx) {
    ModeArgs A; A.budget = Cp.budget; A.fp = &Fp;
    tree_step_body<G, kModeFpu | kModeCap>(E, A, do_expand, do_select, sim_idx);
}
template <class G>
__global__ void __launch_bounds__(256) k_fpu_forced_step(EngineDev E, ForcedDev F, FpuDev Fp, int do_expand, int do_select, u32 sim_idx) {
    ModeArgs A; A.fo = &F; A.fp = &Fp;
    tree_step_body<G, kModeFpu | kModeForced>(E, A, do_expand, do_select, sim_idx);
}
template <class G>
__global__ void __launch_bounds__(256) k_fpu_forced_cap_step(EngineDev E, CapDev Cp, ForcedDev F, FpuDev Fp, int do_expand, int do_select,
                                                             u32 sim_idx) {
    ModeArgs A; A.budget = Cp.budget; A.fo = &F; A.fp = &Fp;
    tree_step_body<G, kModeFpu | kModeForced | kModeCap>(E, A, do_expand, do_select, sim_idx);
}

// The tree steps with proven wins, losses and draws: k_tree_step / k_cap_step with the solver's select rule and
// the proof pass behind the backup.
template <class G>
__global__ void __launch_bounds__(256) k_solve_step(EngineDev E, SolveDev Sv, int do_expand, int do_select, u32 sim_idx) {
    ModeArgs A; A.sv = &Sv;
    tree_step_body<G, kModeSolve>(E, A, do_expand, do_select, sim_idx);
}
template <class G>
__global__ void __launch_bounds__(256) k_solve_cap_step(EngineDev E, CapDev Cp, SolveDev Sv, int do_expand, int do_select, u32 sim_idx) {
    ModeArgs A; A.budget = Cp.budget; A.sv = &Sv;
    tree_step_body<G, kModeSolve | kModeCap>(E, A, do_expand, do_select, sim_idx);
}

// The tree steps with exact early stop: k_tree_step / k_fpu_step with the stop rule between the backup and the walk.
template <class G>
__global__ void __launch_bounds__(256) k_stop_step(EngineDev E, StopDev Sp, int do_expand, int do_select, u32 sim_idx) {
    ModeArgs A; A.sp = &Sp;
    tree_step_body<G, kModeStop>(E, A, do_expand, do_select, sim_idx);
}
template <class G>
__global__ void __launch_bounds__(256) k_fpu_stop_step(EngineDev E, FpuDev Fp, StopDev Sp, int do_expand, int do_select, u32 sim_idx) {
    ModeArgs A; A.fp = &Fp; A.sp = &Sp;
    tree_step_body<G, kModeFpu | kModeStop>(E, A, do_expand, do_select, sim_idx);
}
// ... and the reset of their buffer behind k_root_begin: a slot with a root to search runs its whole budget until the rule says
// otherwise, every other slot sits the search out; no step has walked yet.
__global__ void __launch_bounds__(256) k_stop_begin(EngineDev E, StopDev Sp) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g == 0) Sp.walked[0] = 0u;
    if (g < E.B) Sp.stop_at[g] = E.leaf_kind[(size_t)g * E.K] != LEAF_NONE ? (u32)E.sims : 0u;
}

// Leaf-parallel tree step (K = E.K > 1 leaves per game per step with virtual loss), G::GW lanes per game as
// in k_tree_step.  One launch: [expand the pending leaves of the previous step in ascending j, each followed by the backup
// of its path] then [K' = min(K, sims - sim_idx) walks in ascending j, each leaving a virtual loss (N += 1, W -= 1) on its
// path before the next one starts].  Expanding leaf j and backing up path j before leaf j + 1 gives the bits of "expand all,
// then back up all": an expansion writes only new edges and the header of its own node.  K paths overlap, so unlike
// k_tree_step's pure-store backup every backup and virtual loss is a read-modify-write of the edge's {w0, W}, fenced per path.
template <class G>
__global__ void __launch_bounds__(256) k_leaf_step(EngineDev E, int do_expand, int do_select, u32 sim_idx) {
    constexpr int kGW = G::GW;
    const ModeArgs none;  // (this kernel's mode reads no argument)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int g = t / kGW, sub = t % kGW;
    const int K = E.K;
    Cnt c = {};
    Stamps st; st.start();
    __shared__ u32 s_need, s_base;
    if (threadIdx.x == 0) s_need = 0;
    __syncthreads();
    u32 eval_mask = 0, my_rank = 0;  // lead lane: the walks whose leaf needs an evaluator row; their first rank in the workgroup
    u32 n_coll = 0;                  // lead lane: walks that collided
    if (g < E.B) {
        Edge* const edges = E.edges + (size_t)g * E.ecap;
        LeafRec* const lr = E.lrec + (size_t)g * K;
        const size_t r0 = (size_t)g * K;
        // this game's rows, as per-lane pointers: the kernel-argument bases are not kept live across the walks
        int maxd = E.maxd;
        pin(maxd);  // (a VGPR: SGPRs are the scarce register file of this kernel)
        PathEnt* const path_g = E.path + r0 * maxd;
        u64* const lown = E.leaf_own + r0;
        u64* const lopp = E.leaf_opp + r0;
        uint8_t* const lkind = E.leaf_kind + r0;
        const GameHot hot = E.hot[g];
        const int state = E.g_state[g];
        const bool active = state == 0 && lr[0].kind != LEAF_NONE;  // (a live game always has walk 0's leaf or a READY root)
        u32 ne = hot.n_edges, nn = hot.n_nodes;
        int root_n = (int)hot.root_n;
        if (do_expand) {
            for (int j = 0; j < K; ++j) {
                const LeafRec L = lr[j];
                if (L.kind != LEAF_EVAL && L.kind != LEAF_TERMINAL && L.kind != LEAF_COLLIDE) continue;
                float v;
                const u32 e0 = ne; int n = 0;
                if (L.kind == LEAF_EVAL) {
                    const u32 row = E.compact ? L.slot : (u32)(r0 + j);
                    LogitSrc ls; ls.kind = BZ_EVAL_EXTERNAL; ls.h = 0; ls.row = E.logits + (size_t)row * G::NA;
                    v = E.value[row];
                    if (sub == 0 && !(v >= -3.0e38f && v <= 3.0e38f)) atomicOr(&E.flags[FLAG_ERR], ERR_EVAL_NONFINITE);
                    n = dev_expand<G>(E, g, sub, L.node, L.legal, L.info, ls, ne, c, st);
                    if (sub == 0) { c.v[CNT_NET_LEAVES]++; lr[j].v = v; }
                    if (L.node == 0) root_n = n;
                } else if (L.kind == LEAF_COLLIDE) {  // the value of the node an earlier walk of the step created, expanded above
                    group_fence();
                    v = 0.0f;  // (stays 0 without a source: a node left without edges by ERR_EDGE_OVERFLOW)
                    for (int i = 0; i < j; ++i) {
                        const LeafRec S = lr[i];
                        if (S.kind == LEAF_EVAL && S.node == L.node) v = S.v;
                    }
                } else {
                    v = (float)((int)((L.info >> 9) & 3u) - 1);
                }
                group_fence();  // this game's earlier expansions and backups -> the loads below
                const PathEnt* path = path_g + (size_t)j * maxd;
                const int depth = (int)L.depth, dmax = depth < maxd ? depth : maxd;
                for (int d = sub; d < dmax; d += kGW) {  // val = -v at the leaf's edge; W = (W + 1) + val; N stays
                    const PathEnt pe = path[d];
                    const float val = ((dmax - 1 - d) & 1) ? v : -v;
                    uint2 w = *reinterpret_cast<const uint2*>(edges + pe.eidx);
                    if (d == depth - 1 && n > 0) {
                        w.x |= (u32)n << kNchShift;
                        edges[pe.eidx].w3 = L.node | (e0 << kChildBits);
                    }
                    w.y = __float_as_uint((__uint_as_float(w.y) + 1.0f) + val);
                    *reinterpret_cast<uint2*>(edges + pe.eidx) = w;
                }
                if (sub == 0) c.v[CNT_EDGES_BACKED] += (u32)dmax;
            }
            if (sub == 0) { E.hot[g].n_edges = ne; E.hot[g].root_n = (u32)root_n; }
        }
        st.mark(2);
        if (do_select) {
            int kp = E.sims - (int)sim_idx < K ? E.sims - (int)sim_idx : K;
            pin(kp);
            const u32 sum0 = sim_idx + (E.reuse ? hot.root_base : 0u);  // the root's visits when walk 0 starts
            const u64 rown = E.g_own[g], ropp = E.g_opp[g];
            const int rtm = E.g_to_move[g];
            for (int j = 0; j < K; ++j) {
                u32 kind_out = LEAF_NONE;
                if (active && j < kp) {
                    group_fence();  // edges and virtual losses written above are read by this walk
                    u32 leaf2; int k2, depth; float tv;
                    LeafPos lpos; lpos.own = 0; lpos.opp = 0; lpos.legal = 0; lpos.info = 0; lpos.src = 0; lpos.src_e0 = 0;
                    RootRef root; root.own = rown; root.opp = ropp; root.tm = rtm; root.n = root_n;
                    root.sumN = sum0 + (u32)j;  // walks started so far, pending ones included
                    root.has_pre = false; root.pre.w0 = 0; root.pre.W = 0.0f; root.pre.P = 0.0f; root.pre.w3 = 0;
                    root.tt_gen = 0; root.prev_nodes = 0;
                    PathEnt* path = path_g + (size_t)j * maxd;
                    PathHbm<kGW> sink; sink.p = path; sink.mine.eidx = 0; sink.mine.w0 = 0; sink.mine.W = 0.0f; sink.mine.pad = 0;
                    dev_select<G, kModeLeaf>(E, g, sub, root, nn, leaf2, k2, depth, tv, c, sink, lpos, st, none, 0.0f, 0.0f);
                    sink.flush(sub, depth);
                    group_fence();  // the walk's child-creation stores and deep path entries -> the virtual loss below
                    // virtual loss: N += 1, W -= 1 on every path edge, from the words the walk saw (nothing else wrote them since)
                    const int dmax = depth < maxd ? depth : maxd;
                    if (sub < dmax)
                        *reinterpret_cast<uint2*>(edges + sink.mine.eidx) = make_uint2(sink.mine.w0 + 1u, __float_as_uint(sink.mine.W - 1.0f));
                    for (int d = sub + kGW; d < dmax; d += kGW) {
                        const PathEnt pe = path[d];
                        *reinterpret_cast<uint2*>(edges + pe.eidx) = make_uint2(pe.w0 + 1u, __float_as_uint(pe.W - 1.0f));
                    }
                    if (sub == 0) {
                        LeafRec R; R.legal = 0; R.node = leaf2; R.info = 0; R.slot = 0; R.depth = (u32)depth; R.kind = (u32)k2; R.v = 0.0f;
                        if (k2 == LEAF_EVAL) {
                            R.legal = lpos.legal; R.info = lpos.info;
                            lown[j] = lpos.own; lopp[j] = lpos.opp;
                            if (E.compact) eval_mask |= 1u << j;
                        } else if (k2 == LEAF_COLLIDE) {  // (the walk that created the node is found at expansion)
                            n_coll++;
                        } else {  // terminal leaf: the backup needs its value only
                            R.info = (u32)((int)tv + 1) << 9;
                        }
                        lr[j] = R;
                    }
                    kind_out = (u32)k2;
                } else if (sub == 0) {
                    lr[j].kind = LEAF_NONE;
                }
                if (sub == 0) lkind[j] = (uint8_t)kind_out;
            }
            if (sub == 0) E.hot[g].n_nodes = nn;
            if (sub == 0 && eval_mask) my_rank = atomicAdd(&s_need, (u32)__popc(eval_mask));
            // the packed-leaf counters alternate step by step (computed here, not kept live across the walks)
            if (t == 0) E.flags[FLAG_NEVAL + ((sim_idx / (u32)K + 1u) & 1u)] = 0;  // the buffer the NEXT select packs into
        } else if (t == 0) {  // expand-only step (end of a search / step API): nothing is packed any more
            E.flags[FLAG_NEVAL] = 0; E.flags[FLAG_NEVAL + 1] = 0;
        }
    }
    if (do_select && E.compact) {  // (kernel arguments: the whole grid takes this branch or none of it)
        __syncthreads();
        if (threadIdx.x == 0) s_base = s_need ? atomicAdd(&E.flags[FLAG_NEVAL + ((sim_idx / (u32)E.K) & 1u)], s_need) : 0u;
        __syncthreads();
        if (eval_mask) {  // (lead lanes only)
            u32 slot = s_base + my_rank;
            LeafRec* const lr = E.lrec + (size_t)g * K;
            for (u32 m = eval_mask; m; m &= m - 1u) {
                const int j = __builtin_ctz(m);
                const size_t r = (size_t)g * K + j;
                lr[j].slot = slot; E.c_own[slot] = E.leaf_own[r]; E.c_opp[slot] = E.leaf_opp[r];
                ++slot;
            }
        }
    }
    st.mark(5);
    {
        u32 x = n_coll;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
        if ((threadIdx.x & 63) == 0 && x) atomicAdd(reinterpret_cast<unsigned long long*>(E.counters) + kCntCollisions, (unsigned long long)x);
    }
    cnt_flush<G::GW>(E, c);
    st.mark(6);
    st.flush(E.counters);
}

// whole search in one launch for the synthetic evaluators (BASELINE cfg 2):
// root expansion + sims x (select, expand, backup), no host round trip.  The dependent-access
// chain per simulation is what bounds this kernel (every game of the batch is in flight at once,
// one lane group per game), so it is kept as short as the data structure allows: the select path
// lives in LDS together with the N and W it saw (backup = stores only), the created leaf's position
// and legal mask come back from the walk in registers (expansion reads nothing), and the group's
// store -> load ordering is a wavefront-scope fence (no wait for store round trips).
template <class G>
__global__ void __launch_bounds__(256) k_search_fused(EngineDev E, int eval_kind) {
    constexpr int kGW = G::GW, kGPB = 256 / kGW;
    const ModeArgs none;  // (this kernel's mode reads no argument)
    __shared__ PathEntLds s_path[kGPB][G::MAXD];
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int g = t / kGW, sub = t % kGW;
    PathEntLds* mypath = s_path[threadIdx.x / kGW];
    Cnt c = {};
    if (g < E.B && E.g_state[g] == 0) {
        bool ok = true;
        if (sub == 0) ok = dev_root_init<G>(E, g);
        ok = __shfl((int)ok, 0, kGW) != 0;
        if (ok) {
            u32 nn = 1, ne = 0;
            LogitSrc ls; ls.kind = eval_kind; ls.row = nullptr;
            RootRef root; root.own = E.g_own[g]; root.opp = E.g_opp[g]; root.tm = E.g_to_move[g];
            root.has_pre = false; root.pre.w0 = 0; root.pre.W = 0.0f; root.pre.P = 0.0f; root.pre.w3 = 0;
            ls.h = hash_pos(root.own, root.opp);
            group_fence();
            Stamps st; st.start();
            root.n = dev_expand<G>(E, g, sub, 0, G::legal(root.own, root.opp), (root.tm == 1 ? 1u : 0u) << 11, ls, ne, c, st);
            if (sub == 0) E.hot[g].root_n = (u32)root.n;
            PathLds sink{mypath};
            for (int s = 0; s < E.sims; ++s) {
                group_fence();  // this group's stores -> its loads
                u32 leaf; int kind, depth; float v;
                LeafPos lp; lp.own = 0; lp.opp = 0; lp.legal = 0; lp.info = 0;
                root.sumN = (u32)s;
                dev_select<G, 0u>(E, g, sub, root, nn, leaf, kind, depth, v, c, sink, lp, st, none, 0.0f, 0.0f);
                u32 e0 = ne; int n = 0;
                if (kind == LEAF_EVAL) {
                    ls.h = hash_pos(lp.own, lp.opp);
                    n = dev_expand<G>(E, g, sub, leaf, lp.legal, lp.info, ls, ne, c, st);
                    v = eval_kind == BZ_EVAL_HASH ? hash_value(ls.h) : 0.0f;
                }
                group_fence();  // LDS path entries (lane 0) -> the lanes that back them up
                dev_backup<G::GW>(E, g, sub, depth, v, mypath, leaf, e0, n, c);
            }
            if (sub == 0) { E.hot[g].n_nodes = nn; E.hot[g].n_edges = ne; }
        }
    }
    cnt_flush<G::GW>(E, c);
}

// ---- Tic-tac-toe specialisation of the fused search (BASELINE cfg 2; sims <= 120).
// The walk is a dependent chain per game and every game of the batch is in flight at once, so the
// time of a launch is sims x (dependent memory round trips per simulation).  Three things cut the chain:
//  * the root's edges live in REGISTERS for the whole search (lane sub holds edges sub, sub+GW, ...): level 0
//    of every simulation reads nothing, its backup writes nothing; the edges go to HBM once, at the end;
//  * an edge's `ca` word also carries what the walk needs to know about the child -- its first edge, its
//    child count, terminal flag and value -- so a level is ONE load (the child's edges), never the child's
//    node first (TTT's numbers fit in ONE word: child 8 | edge0 12 | n 4 | action 4 | terminal 1 | value 2 in w3,
//    with w0 a plain visit count -- this kernel's private edge record, EdgeFmtTttFused);
//  * positions are carried down the walk by applying the actions (TTT: swap + one bit), so nodes below the
//    root are never loaded -- and, since nothing reads them, never stored.
// Results (root statistics, counters, examples) are bit-identical to the generic kernel and the oracle; the
// root edges are written back as the engine's packed record, which is all that k_play / k_root_stats read.
__device__ __forceinline__ u32 ttt_ca(u32 child, u32 edge0, u32 n, u32 act, bool term, int tv) {
    return child | (edge0 << 8) | (n << 20) | (act << 24) | ((term ? 1u : 0u) << 28) | ((u32)(tv + 1) << 29);
}
constexpr int kTttFusedMaxSims = 120;

__device__ __forceinline__ float puct_score(const Edge& e, float c_puct, float sq) {
    float q = e.w0 > 0 ? fdiv(e.W, (float)e.w0) : 0.0f;
    float u = c_puct * e.P;
    u = u * sq;
    u = fdiv(u, 1.0f + (float)e.w0);
    return q + u;
}

// kUniform = the uniform evaluator (cfg 2) at compile time: the kernel is at ~90 % of its SIMDs' issue slots, so the
// exponentials, the serial softmax sum and the position hash it does not need are time, not just instructions.
template <int kGW, bool kUniform>
__global__ void __launch_bounds__(256) k_search_fused_ttt(EngineDev E) {
    using G = TicTacToe;
    constexpr int eval_kind = kUniform ? BZ_EVAL_UNIFORM : BZ_EVAL_HASH;
    constexpr int kGPB = 256 / kGW, kCH = (G::MAXCH + kGW - 1) / kGW;
    __shared__ PathEntLds s_path[kGPB][G::MAXD];
    // sqrt(max(visits, 1)) for every visit count this kernel can see (sims <= 120): the correctly rounded square root is
    // ~20 instructions, the table one LDS read -- and holds the very values fsqrt() returns
    __shared__ float s_sqrt[128];
    if (threadIdx.x < 128) s_sqrt[threadIdx.x] = fsqrt((float)(threadIdx.x > 1 ? threadIdx.x : 1));
    __syncthreads();
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int g = t / kGW, sub = t % kGW;
    PathEntLds* mypath = s_path[threadIdx.x / kGW];
    Cnt c = {};
    if (g < E.B && E.g_state[g] == 0) {
        bool ok = true;
        if (sub == 0) ok = dev_root_init<G>(E, g);
        ok = __shfl((int)ok, 0, kGW) != 0;
        if (ok) {
            Edge* edges = E.edges + (size_t)g * E.ecap;
            const bool lead = sub == 0;
            u32 nn = 1, ne = 0;
            LogitSrc ls; ls.kind = eval_kind; ls.row = nullptr;
            const u64 rown = E.g_own[g], ropp = E.g_opp[g];
            const int rtm = E.g_to_move[g];
            ls.h = kUniform ? 0 : hash_pos(rown, ropp);
            group_fence();
            Stamps st; st.start();
            dev_expand<G, kGW, true, EdgeFmtTttFused, kUniform>(E, g, sub, 0, G::legal(rown, ropp), (rtm == 1 ? 1u : 0u) << 11, ls, ne, c, st);
            group_fence();
            const int rn = (int)ne;  // the root's children (>= 1: a terminal root was refused above)
            Edge re[kCH];
            // Q = W / N and c_puct * P of the register-resident root edges are kept next to them: Q changes only for the
            // edge a simulation backs up (one correctly rounded division per simulation instead of one per root edge),
            // c_puct * P never.  The values are the ones puct_score would recompute, bit for bit.
            float rq[kCH], rcp[kCH];
#pragma unroll
            for (int k = 0; k < kCH; ++k) {
                const int i = sub + kGW * k;
                if (i < rn) re[k] = edges[i];
                else { re[k].w0 = 0; re[k].W = 0.0f; re[k].P = 0.0f; re[k].w3 = 0; }
                rq[k] = re[k].w0 > 0 ? fdiv(re[k].W, (float)re[k].w0) : 0.0f;
                rcp[k] = E.c_puct * re[k].P;
            }
            for (int s = 0; s < E.sims; ++s) {
                group_fence();  // this group's stores of the previous simulation -> its loads
                // ---- level 0 from registers
                // (first maximum = highest score, lowest child index on ties: every lane scans its own edges in ascending
                // order, then ONE exchange across the group's lanes -- the order of the comparisons does not matter)
                float bestW = 0.0f; int best = 0; u32 bestN = 0, bestca = 0;
                {
                    const float sq = s_sqrt[s];
                    Cand lb; lb.sc = -__builtin_inff(); lb.i = sub; lb.w0 = 0; lb.w3 = 0; lb.W = 0.0f;
#pragma unroll
                    for (int k = 0; k < kCH; ++k) {
                        const int i = sub + kGW * k;
                        if (i < rn) {  // puct_score with the cached terms
                            float u = rcp[k] * sq;
                            u = fdiv(u, 1.0f + (float)re[k].w0);
                            const float sc = rq[k] + u;
                            if (sc > lb.sc) { lb.sc = sc; lb.i = i; lb.w0 = re[k].w0; lb.w3 = re[k].w3; lb.W = re[k].W; }
                        }
                    }
                    group_argmax<kGW>(lb);
                    best = lb.i; bestN = lb.w0; bestca = lb.w3; bestW = lb.W;
                }
                if (lead) { c.v[CNT_SIMS]++; c.v[CNT_PATH_NODES]++; c.v[CNT_CHILD_SCORED] += (u32)rn; }
                const int i0 = best; const u32 N0 = bestN; const float W0 = bestW;
                int depth = 1;
                u64 own = rown, opp = ropp; int tm = rtm;
                u32 ca = bestca, parentN = bestN, pe_idx = (u32)best, new_ca = 0;
                bool made = false;
                float v = 0.0f;
                for (;;) {  // walk below the root: `ca` is the edge just chosen
                    const int act = (int)((ca >> 24) & 0xFu);
                    u64 cown, copp;
                    G::apply(own, opp, act, &cown, &copp);
                    own = cown; opp = copp; tm = -tm;
                    if (ca & 0xFFu) {  // the child exists
                        if (lead) c.v[CNT_PATH_NODES]++;
                        if ((ca >> 28) & 1u) { v = (float)((int)((ca >> 29) & 3u) - 1); break; }  // terminal, revisited
                        const u32 e0 = (ca >> 8) & 0xFFFu; const int n = (int)((ca >> 20) & 0xFu);
                        const u32 sumN = parentN - 1u;  // visits of the child's edges = visits into it minus the creating one
                        const float sq = s_sqrt[sumN & 127u];
                        const Edge* ed = edges + e0;
                        Cand lb; lb.sc = -__builtin_inff(); lb.i = sub; lb.w0 = 0; lb.w3 = 0; lb.W = 0.0f;
#pragma unroll
                        for (int k = 0; k < kCH; ++k) {
                            const int i = sub + kGW * k;
                            if (i < n) {
                                const Edge e = ed[i];
                                const float sc = puct_score(e, E.c_puct, sq);
                                if (sc > lb.sc) { lb.sc = sc; lb.i = i; lb.w0 = e.w0; lb.w3 = e.w3; lb.W = e.W; }
                            }
                        }
                        group_argmax<kGW>(lb);
                        best = lb.i; bestN = lb.w0; bestca = lb.w3; bestW = lb.W;
                        pe_idx = e0 + (u32)best;
                        if (lead) {
                            c.v[CNT_CHILD_SCORED] += (u32)n;
                            if (depth < E.maxd) { PathEntLds pe; pe.eidx = pe_idx; pe.w0 = bestN; pe.W = bestW; mypath[depth] = pe; }
                            else atomicOr(&E.flags[FLAG_ERR], ERR_DEPTH);
                        }
                        depth++;
                        ca = bestca; parentN = bestN;
                        continue;
                    }
                    // create the child behind the chosen edge (env step) and, unless terminal, expand it at once
                    const u32 id = nn++;
                    const u64 lg = G::legal(own, opp);
                    int tv = 0;
                    const bool term = G::terminal(own, opp, tm, lg, &tv);
                    if (lead) { c.v[CNT_ENV_STEPS]++; c.v[CNT_PATH_NODES]++; }
                    if (term) {
                        new_ca = ttt_ca(id, 0, 0, (u32)act, true, tv);
                        v = (float)tv;
                    } else {
                        ls.h = kUniform ? 0 : hash_pos(own, opp);
                        const u32 e0 = ne;
                        dev_expand<G, kGW, false, EdgeFmtTttFused, kUniform>(E, g, sub, id, lg, 0, ls, ne, c, st);
                        new_ca = ttt_ca(id, e0, ne - e0, (u32)act, false, 0);
                        v = eval_kind == BZ_EVAL_HASH ? hash_value(ls.h) : 0.0f;
                    }
                    made = true;
                    break;
                }
                if (made && depth > 1 && lead) edges[pe_idx].w3 = new_ca;  // (depth 1: the parent edge is a root register)
                // ---- backup: root edge in registers, deeper edges by one 8-byte store each from the LDS path
                const int dmax = depth < E.maxd ? depth : E.maxd;
                {
                    const float val0 = ((dmax - 1) & 1) ? v : -v;
#pragma unroll
                    for (int k = 0; k < kCH; ++k)
                        if (sub + kGW * k == i0) {
                            re[k].w0 = N0 + 1u; re[k].W = W0 + val0;
                            rq[k] = fdiv(re[k].W, (float)re[k].w0);
                            if (made && depth == 1) re[k].w3 = new_ca;
                        }
                }
                group_fence();  // the lead lane's LDS path entries -> the lanes that back them up
                for (int d = sub; d < dmax; d += kGW) {
                    if (d == 0) continue;
                    PathEntLds pe = mypath[d];
                    float val = ((dmax - 1 - d) & 1) ? v : -v;
                    *reinterpret_cast<uint2*>(edges + pe.eidx) = make_uint2(pe.w0 + 1u, __float_as_uint(pe.W + val));
                }
                if (lead) c.v[CNT_EDGES_BACKED] += (u32)dmax;
            }
            // root edges back to HBM as the engine's packed record (N | action, child id): what k_play / k_root_stats read
#pragma unroll
            for (int k = 0; k < kCH; ++k) {
                const int i = sub + kGW * k;
                if (i < rn) { Edge e = re[k]; e.w0 = e.w0 | (((e.w3 >> 24) & 0xFu) << kActShift); e.w3 = e.w3 & 0xFFu; edges[i] = e; }
            }
            if (lead) { E.hot[g].n_nodes = nn; E.hot[g].n_edges = ne; E.hot[g].root_n = (u32)rn; }
        }
    }
    cnt_flush<kGW>(E, c);
}

template <class G>
__global__ void __launch_bounds__(256) k_root_stats(EngineDev E) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B) return;
    u32* rn = E.root_N + (size_t)g * G::NA; float* rw = E.root_W + (size_t)g * G::NA; float* rp = E.root_P + (size_t)g * G::NA;
    for (int a = 0; a < G::NA; ++a) { rn[a] = 0; rw[a] = 0.0f; rp[a] = 0.0f; }
    if (E.g_state[g] != 0) return;
    Node r = E.nodes[(size_t)g * E.ncap];
    const Edge* ed = E.edges + (size_t)g * E.ecap + r.edge0;
    for (int i = 0; i < (int)(r.info & 0xFFu); ++i) {
        Edge e = ed[i];
        int a = e_action(e.w0);
        rn[a] = e_N(e.w0); rw[a] = e.W; rp[a] = e.P;
    }
}

// M5's move choice, shared by k_play and k_root_policy: pi = N / sum N at the edges' actions (0 elsewhere)
// and the index of the played edge -- tau = 1 (made < temp_moves): sampled ~ N with the counter RNG (seed, game id, moves
// made), else the first maximum of N
// (kPi = false: the choice alone, pi is not touched -- a fast search under playout cap randomisation)
template <class G, bool kPi = true>
__device__ __forceinline__ int dev_puct_choice(const EngineDev& E, int g, const Edge* ed, int n, u32 sumN, int made, int round,
                                               float* pi) {
    if (kPi) for (int a = 0; a < G::NA; ++a) pi[a] = 0.0f;
    int pick = 0;
    if (made < E.temp_moves) {  // tau = 1: sample ~ N with the counter RNG (seed, game id, moves made)
        u64 gid = E.id_base + (u64)round * E.id_stride + (u64)g;
        u64 rr = rng_draw(E.seed, gid, (u64)made) % (u64)sumN, cum = 0;
        bool found = false;
        for (int i = 0; i < n; ++i) {
            const u32 w0 = ed[i].w0, N = e_N(w0);
            if (kPi) pi[e_action(w0)] = fdiv((float)N, (float)sumN);
            cum += N;
            if (!found && cum > rr) { pick = i; found = true; }
        }
    } else {  // tau = 0: argmax N, ties -> lowest action
        u32 bn = 0;
        for (int i = 0; i < n; ++i) {
            const u32 w0 = ed[i].w0, N = e_N(w0);
            if (kPi) pi[e_action(w0)] = fdiv((float)N, (float)sumN);
            if (N > bn) { bn = N; pick = i; }
        }
    }
    return pick;
}

// The Gumbel move choice, shared by k_gumbel_play and k_root_policy: pi = softmax(logf(P~) + sigma) at the
// edges' actions (0 elsewhere; the softmax sequence of DESIGN.md 3.5) and the index of the played edge, the first maximum of
// base + sigma among the edges with N = max N
template <class G>
__device__ __forceinline__ int dev_gumbel_choice(const GumbelDev& Gm, int g, const Edge* ed, int n, float* pi) {
    for (int a = 0; a < G::NA; ++a) pi[a] = 0.0f;
    const GumbelStats st = gumbel_stats(Gm, ed, n, Gm.vroot[g]);
    const float* base = Gm.base + (size_t)g * G::MAXCH;
    int pick = -1;
    float bests = 0.0f, m = 0.0f;
    for (int i = 0; i < n; ++i) {
        const Edge e = ed[i];
        const float sg = gumbel_sigma(st, gumbel_cq(e, st.vmix));
        const float x = logf_spec(gumbel_pfloor(e.P)) + sg;
        m = (i == 0 || x > m) ? x : m;
        if (e_N(e.w0) == st.nmax) {
            const float sc = base[i] + sg;
            if (pick < 0 || sc > bests) { pick = i; bests = sc; }
        }
        pi[e_action(e.w0)] = x;  // (the logit for now: exponentiated below)
    }
    float s = 0.0f;
    for (int i = 0; i < n; ++i) {
        float* p = pi + e_action(ed[i].w0);
        const float ex = expf_spec(*p - m);
        *p = ex;
        s = s + ex;
    }
    for (int i = 0; i < n; ++i) {
        float* p = pi + e_action(ed[i].w0);
        *p = fdiv(*p, s);
    }
    return pick < 0 ? 0 : pick;
}

// M5's rest after the choice of root edge `pick`: example row, env step, pass rule (reversi_terminal.py:31-35), terminal
// handling, z back-fill (k_play, k_gumbel_play and k_cap_play).  record = false: the move is played but no row is written and
// nex does not advance (a fast search); a game may then finish with ex_len = 0
template <class G>
__device__ __forceinline__ void dev_play_tail(const EngineDev& E, int g, const Node& root, const Edge* ed, int pick, int round,
                                              int nex, int made, int tm, size_t rowbase, size_t row, int restart, bool record = true) {
    const Edge pk = ed[pick];
    int a = e_action(pk.w0);
    u32 keep_node = e_child(pk.w3), keep_N = e_N(pk.w0);  // subtree reuse: the chosen child and its visits
    if (record) {
        E.ex_own[row] = root.own; E.ex_opp[row] = root.opp; E.ex_mover[row] = (int8_t)tm; E.ex_act[row] = (uint8_t)a;
        nex++;
    }
    u64 own, opp;
    G::apply(root.own, root.opp, a, &own, &opp);
    tm = -tm; made++;
    u64 lg = G::legal(own, opp);
    int tv;
    if (G::terminal(own, opp, tm, lg, &tv)) {
        int w = tv * tm;
        for (int t = 0; t < nex; ++t) E.ex_z[rowbase + t] = (int8_t)(w * E.ex_mover[rowbase + t]);
        E.ex_len[(size_t)round * E.B + g] = nex;
        E.ex_winner[(size_t)round * E.B + g] = (int8_t)w;
        atomicAdd(&E.flags[FLAG_FINISHED], 1u);
        if (restart && round + 1 < E.rounds) { dev_start_game<G>(E, g, round + 1); return; }
        E.g_state[g] = 1;
    } else if (lg == 0) {  // the next mover cannot move: flip the side again
        u64 t = own; own = opp; opp = t; tm = -tm;
        E.g_passes[g]++;
        if (E.reuse && keep_node) {  // the kept root lies behind the child's only edge, the pass
            const Node cn = E.nodes[(size_t)g * E.ncap + keep_node];
            const Edge pe = E.edges[(size_t)g * E.ecap + cn.edge0];
            keep_node = e_child(pe.w3); keep_N = e_N(pe.w0);
        }
    }
    if (E.reuse) {  // keep the subtree iff it exists and the next search cannot outgrow the arena
        const bool ok = keep_node != 0 && keep_N + (u32)E.sims + 2u <= (u32)E.ncap;
        E.g_reuse[g] = ok ? keep_node : 0u;
        E.hot[g].root_base = ok ? keep_N - 1u : 0u;
    }
    E.g_own[g] = own; E.g_opp[g] = opp; E.g_to_move[g] = (int8_t)tm; E.g_moves[g] = made; E.g_nex[g] = nex;
}

// The move of a search with proven edges, shared by k_solve_play, k_solve_cap_play and k_root_policy: pi stays
// N / sum N (dev_puct_choice writes it), the played edge is solver_pick's
template <class G, bool kPi = true>
__device__ __forceinline__ int dev_solver_choice(const EngineDev& E, int g, const Edge* ed, int n, u32 sumN, int made, int round,
                                                 float* pi) {
    const int plain = dev_puct_choice<G, kPi>(E, g, ed, n, sumN, made, round, pi);
    bool any = false;
    for (int i = 0; i < n; ++i) any = any || e_decided(ed[i].w0);
    if (!any) return plain;
    const bool tau1 = made < E.temp_moves;
    const u64 gid = E.id_base + (u64)round * E.id_stride + (u64)g;
    return solver_pick(n, [ed](int i) { return (u64)e_N(ed[i].w0); }, [ed](int i) { return e_cval(ed[i].w0); }, tau1,
                       tau1 ? rng_draw(E.seed, gid, (u64)made) : 0ULL);
}

// the proof state of every slot's root: edge_out [B][NA] the decided value of the edge of every action (2:
// undecided or no such edge), root_out [B] the root's recorded value (2: undecided; idle slots: all 2)
template <class G>
__global__ void __launch_bounds__(256) k_solve_read(EngineDev E, SolveDev Sv, int8_t* edge_out, int8_t* root_out) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B) return;
    int8_t* eo = edge_out + (size_t)g * G::NA;
    for (int a = 0; a < G::NA; ++a) eo[a] = (int8_t)kSolverUndecided;
    root_out[g] = (int8_t)kSolverUndecided;
    if (E.g_state[g] != 0) return;
    const Node r = E.nodes[(size_t)g * E.ncap];
    const Edge* ed = E.edges + (size_t)g * E.ecap + r.edge0;
    for (int i = 0; i < (int)(r.info & 0xFFu); ++i) { const u32 w0 = ed[i].w0; eo[e_action(w0)] = (int8_t)e_cval(w0); }
    const int rec = Sv.root[g];
    if (rec != 0) root_out[g] = (int8_t)(rec - 2);
}

// The move and the pi of a search with forced playouts: the DESIGN.md 3.7 choice over the raw N; pi from the
// pruned N' (F.prune) or the raw N.  pi = nullptr: the choice alone.
template <class G>
__device__ __forceinline__ int dev_forced_choice(const EngineDev& E, const ForcedDev& F, int g, const Edge* ed, int n, u32 sumN,
                                                 int made, int round, float* pi) {
    const int pick = dev_puct_choice<G, false>(E, g, ed, n, sumN, made, round, nullptr);
    if (pi) {
        for (int a = 0; a < G::NA; ++a) pi[a] = 0.0f;
        const auto sink = [pi](int, const Edge& e, u32 Np) { pi[e_action(e.w0)] = (float)Np; };  // (the count for now: divided below)
        u32 S = sumN;
        if (F.prune) S = forced_prune(ed, n, E.c_puct, F.k, sink);
        else for (int i = 0; i < n; ++i) sink(i, ed[i], e_N(ed[i].w0));
        for (int i = 0; i < n; ++i) {
            float* p = pi + e_action(ed[i].w0);
            *p = fdiv(*p, (float)S);
        }
    }
    return pick;
}

// M5 + the reference's turn loop under the search mode M (Mode, above; kModeFpu and kModeGfull change nothing here): pi, move
// choice, example row, env step, pass rule (reversi_terminal.py:31-35), terminal handling, z back-fill.
// kModeGumbel: the improved policy as pi and the Gumbel move.  kModeSolve: dev_solver_choice's move.  kModeForced: the pruned pi in
// the recorded row; the move is the plain one.  kModeCap: only a full search (budget = sims) records its row; a fast one plays its
// move by the same rule (tau = 1 sampling over its own visit sum included; not forced) and writes nothing.
template <class G, unsigned M>
__device__ __forceinline__ void play_body(const EngineDev& E, const ModeArgs& A, int restart) {
    using Md = Mode<M>;
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B || E.g_state[g] != 0) return;
    Node root = E.nodes[(size_t)g * E.ncap];
    const Edge* ed = E.edges + (size_t)g * E.ecap + root.edge0;
    int n = (int)(root.info & 0xFFu);
    [[maybe_unused]] u32 sumN = 0;
    if constexpr (!Md::gumbel) for (int i = 0; i < n; ++i) sumN += e_N(ed[i].w0);
    int round = E.g_round[g], nex = E.g_nex[g], made = E.g_moves[g], tm = E.g_to_move[g];
    const bool full = !Md::cap || A.budget[g] >= (u32)E.sims;
    size_t rowbase = ((size_t)round * E.B + g) * E.t_max;
    if (full && nex >= E.t_max) { atomicOr(&E.flags[FLAG_ERR], ERR_EXAMPLE_OVERFLOW); E.g_state[g] = 1; return; }
    size_t row = rowbase + nex;
    int pick;
    if constexpr (Md::gumbel) pick = dev_gumbel_choice<G>(*A.gm, g, ed, n, E.ex_pi + row * G::NA);
    else if constexpr (Md::forced) pick = dev_forced_choice<G>(E, *A.fo, g, ed, n, sumN, made, round, full ? E.ex_pi + row * G::NA : nullptr);
    else if constexpr (Md::solve) pick = full ? dev_solver_choice<G>(E, g, ed, n, sumN, made, round, E.ex_pi + row * G::NA)
                                              : dev_solver_choice<G, false>(E, g, ed, n, sumN, made, round, nullptr);
    else pick = full ? dev_puct_choice<G>(E, g, ed, n, sumN, made, round, E.ex_pi + row * G::NA)
                     : dev_puct_choice<G, false>(E, g, ed, n, sumN, made, round, nullptr);
    dev_play_tail<G>(E, g, root, ed, pick, round, nex, made, tm, rowbase, row, restart, full);
}
template <class G>
__global__ void __launch_bounds__(256) k_play(EngineDev E, int restart) { play_body<G, 0u>(E, ModeArgs{}, restart); }
template <class G>
__global__ void __launch_bounds__(256) k_gumbel_play(EngineDev E, GumbelDev Gm, int restart) {
    ModeArgs A; A.gm = &Gm;
    play_body<G, kModeGumbel>(E, A, restart);
}
template <class G>
__global__ void __launch_bounds__(256) k_cap_play(EngineDev E, CapDev Cp, int restart) {
    ModeArgs A; A.budget = Cp.budget;
    play_body<G, kModeCap>(E, A, restart);
}
template <class G>
__global__ void __launch_bounds__(256) k_solve_play(EngineDev E, int restart) { play_body<G, kModeSolve>(E, ModeArgs{}, restart); }
template <class G>
__global__ void __launch_bounds__(256) k_solve_cap_play(EngineDev E, CapDev Cp, int restart) {
    ModeArgs A; A.budget = Cp.budget;
    play_body<G, kModeSolve | kModeCap>(E, A, restart);
}
template <class G>
__global__ void __launch_bounds__(256) k_forced_play(EngineDev E, ForcedDev F, int restart) {
    ModeArgs A; A.fo = &F;
    play_body<G, kModeForced>(E, A, restart);
}
template <class G>
__global__ void __launch_bounds__(256) k_forced_cap_play(EngineDev E, CapDev Cp, ForcedDev F, int restart) {
    ModeArgs A; A.budget = Cp.budget; A.fo = &F;
    play_body<G, kModeForced | kModeCap>(E, A, restart);
}

// k_root_policy with forced playouts: the pruned pi and the unchanged action; under the cap (Cp.fast > 0) a
// fast search was not forced and reports its raw pi
template <class G>
__global__ void __launch_bounds__(256) k_forced_root_policy(EngineDev E, CapDev Cp, ForcedDev F, float* pi_out, int32_t* act_out) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B) return;
    float* pi = pi_out + (size_t)g * G::NA;
    const Node root = E.nodes[(size_t)g * E.ncap];
    const Edge* ed = E.edges + (size_t)g * E.ecap + root.edge0;
    const int n = (int)(root.info & 0xFFu);
    if (E.g_state[g] != 0 || n == 0) {  // (n == 0: no search has expanded this slot's root)
        for (int a = 0; a < G::NA; ++a) pi[a] = 0.0f;
        act_out[g] = -1;
        return;
    }
    u32 sumN = 0;
    for (int i = 0; i < n; ++i) sumN += e_N(ed[i].w0);
    ForcedDev Fg = F;
    if (Cp.fast > 0 && Cp.budget[g] < (u32)E.sims) Fg.prune = 0;
    const int pick = dev_forced_choice<G>(E, Fg, g, ed, n, sumN, E.g_moves[g], E.g_round[g], pi);
    act_out[g] = e_action(ed[pick].w0);
}

// the pi and the action bz_engine_play would write and play, into pi [B][NA] / action [B] (idle or finished slots: zeros, -1)
template <class G>
__global__ void __launch_bounds__(256) k_root_policy(EngineDev E, GumbelDev Gm, int solve, float* pi_out, int32_t* act_out) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B) return;
    float* pi = pi_out + (size_t)g * G::NA;
    const Node root = E.nodes[(size_t)g * E.ncap];
    const Edge* ed = E.edges + (size_t)g * E.ecap + root.edge0;
    const int n = (int)(root.info & 0xFFu);
    if (E.g_state[g] != 0 || n == 0) {  // (n == 0: no search has expanded this slot's root)
        for (int a = 0; a < G::NA; ++a) pi[a] = 0.0f;
        act_out[g] = -1;
        return;
    }
    int pick;
    if (Gm.m > 0) {
        pick = dev_gumbel_choice<G>(Gm, g, ed, n, pi);
    } else {
        u32 sumN = 0;
        for (int i = 0; i < n; ++i) sumN += e_N(ed[i].w0);
        pick = solve ? dev_solver_choice<G>(E, g, ed, n, sumN, E.g_moves[g], E.g_round[g], pi)  // 
                     : dev_puct_choice<G>(E, g, ed, n, sumN, E.g_moves[g], E.g_round[g], pi);
    }
    act_out[g] = e_action(ed[pick].w0);
}

// ---- reanalysis: stored rows in, fresh targets out, around one search of the roots they name
// slot g < count searches row r = rows ? rows[first + g] : first + g of the caller's columns (64-bit indices)
__device__ __forceinline__ int64_t dev_reanalyse_row(const int64_t* rows, int64_t first, int g) {
    const int64_t i = first + (int64_t)g;
    return rows ? rows[i] : i;
}
// k_set_roots from example columns: slot g < count becomes a fresh root at row r's boards and mover, every other slot idle.
// A row outside 0 .. n_rows - 1 leaves its slot idle and raises ERR_REANALYSE_ROW; nothing is read at it.  clear != 0: the
// sticky error word and the eval counters start over (k_set_roots' last line), else they stay, so that the chunks of one run
// report together.  Block 0 alone clears and raises, in that order across its barrier: no other block touches the word.
template <class G>
__global__ void __launch_bounds__(256) k_reanalyse_load(EngineDev E, const u64* own, const u64* opp, const int8_t* mover,
                                                        int64_t n_rows, const int64_t* rows, int64_t first, int count, int clear) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0 && clear) { E.flags[FLAG_ERR] = 0; E.flags[FLAG_FINISHED] = 0; E.flags[FLAG_NEVAL] = 0; E.flags[FLAG_NEVAL + 1] = 0; }
        __syncthreads();
        bool bad = false;
        for (int s = threadIdx.x; s < count; s += 256) {
            const int64_t r = dev_reanalyse_row(rows, first, s);
            bad = bad || r < 0 || r >= n_rows;
        }
        if (bad) atomicOr(&E.flags[FLAG_ERR], ERR_REANALYSE_ROW);
    }
    if (g >= E.B) return;
    const int64_t r = g < count ? dev_reanalyse_row(rows, first, g) : -1;
    const bool use = r >= 0 && r < n_rows;
    const int8_t tm = use ? mover[r] : (int8_t)0;
    E.g_own[g] = use ? own[r] : 0ULL; E.g_opp[g] = use ? opp[r] : 0ULL; E.g_to_move[g] = tm;
    E.g_state[g] = tm == 0 ? 1 : 0;
    if (E.reuse) E.g_reuse[g] = 0;
    E.hot[g].root_base = 0;
    E.g_moves[g] = 0; E.g_nex[g] = 0; E.g_round[g] = 0; E.g_passes[g] = 0;
}

// behind the search: row r of slot g < count gets the pi bz_engine_root_policy reports for the slot (k_root_policy's and
// k_forced_root_policy's device functions), q[r] = root_value of the raw visit statistics and kl[r] = surprise_kl of that pi
// against the root edges' priors (no noise is ever drawn here: they are the raw priors); q / kl null: not written.  Idle slots,
// terminal roots (flagged by the search) and unexpanded ones write nothing.  One lane per slot, 64 slots per block: a slot's pi
// is built in the block's shared memory -- the Gumbel softmax reads back what it wrote, and two slots may name one row -- and
// then leaves as whole rows.  Slots that name the same row write the same bits.
template <class G>
__global__ void __launch_bounds__(64) k_reanalyse_store(EngineDev E, GumbelDev Gm, ForcedDev F, int forced, int solve, float* pi_out,
                                                        float* q_out, float* kl_out, int64_t n_rows, const int64_t* rows,
                                                        int64_t first, int count) {
    __shared__ float s_pi[64 * G::NA];
    __shared__ int64_t s_row[64];
    const int lane = threadIdx.x, g = blockIdx.x * 64 + lane;
    int64_t r = -1;
    if (g < E.B && g < count && E.g_state[g] == 0) r = dev_reanalyse_row(rows, first, g);
    if (r >= n_rows) r = -1;
    if (r >= 0) {
        const u64 lg = G::legal(E.g_own[g], E.g_opp[g]);
        int tv;
        if (G::terminal(E.g_own[g], E.g_opp[g], (int)E.g_to_move[g], lg, &tv)) r = -1;  // (its node 0 is an earlier search's)
    }
    if (r >= 0) {
        const Node root = E.nodes[(size_t)g * E.ncap];
        const Edge* ed = E.edges + (size_t)g * E.ecap + root.edge0;
        const int n = (int)(root.info & 0xFFu);
        if (n == 0) {
            r = -1;
        } else {
            float* pi = s_pi + lane * G::NA;
            if (Gm.m > 0 && !forced) {
                dev_gumbel_choice<G>(Gm, g, ed, n, pi);
            } else {
                u32 sumN = 0;
                for (int i = 0; i < n; ++i) sumN += e_N(ed[i].w0);
                if (forced) dev_forced_choice<G>(E, F, g, ed, n, sumN, E.g_moves[g], E.g_round[g], pi);
                else if (solve) dev_solver_choice<G>(E, g, ed, n, sumN, E.g_moves[g], E.g_round[g], pi);
                else dev_puct_choice<G>(E, g, ed, n, sumN, E.g_moves[g], E.g_round[g], pi);
            }
            if (q_out) q_out[r] = root_value(n, [ed](int i) { return e_N(ed[i].w0); }, [ed](int i) { return ed[i].W; });
            if (kl_out) kl_out[r] = surprise_kl(n, [pi, ed](int i) { return pi[e_action(ed[i].w0)]; }, [ed](int i) { return ed[i].P; });
        }
    }
    s_row[lane] = r;
    __syncthreads();
    for (int s = 0; s < 64; ++s) {
        const int64_t rs = s_row[s];
        if (rs < 0) continue;
        float* dst = pi_out + (size_t)rs * G::NA;
        for (int a = lane; a < G::NA; a += 64) dst[a] = s_pi[s * G::NA + a];
    }
}

// Gumbel preparation of every active game's freshly expanded root, in the style of k_root_noise:
// base_i = g_i + logf(P~_i), g_i = scale * -log(-log u) while moves made < temp_moves (and scale > 0), else 0
template <class G>
__global__ void __launch_bounds__(256) k_gumbel_root(EngineDev E, GumbelDev Gm) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B || E.g_state[g] != 0) return;
    const Node r = E.nodes[(size_t)g * E.ncap];
    const int n = (int)(r.info & 0xFFu);
    const Edge* ed = E.edges + (size_t)g * E.ecap + r.edge0;
    float* base = Gm.base + (size_t)g * G::MAXCH;
    const bool noise = E.g_moves[g] < E.temp_moves && Gm.scale > 0.0f;
    const u64 gid = E.id_base + (u64)E.g_round[g] * E.id_stride + (u64)g, ply = (u64)E.g_moves[g];
    for (int i = 0; i < n && i < G::MAXCH; ++i) {
        const float lp = logf_spec(gumbel_pfloor(ed[i].P));
        float gn = 0.0f;
        if (noise) {
            const float u = u01_spec(rng_noise(E.seed ^ 0x6A09E667F3BCC908ULL, gid, ply, (u64)i));
            float y = logf_spec(u);
            y = -y;
            y = logf_spec(y);
            gn = Gm.scale * (-y);
        }
        base[i] = gn + lp;
    }
}

__global__ void __launch_bounds__(256) k_count_active(EngineDev E) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    u32 act = (g < E.B && E.g_state[g] == 0) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) act += __shfl_xor(act, o, 64);
    if ((threadIdx.x & 63) == 0 && act) atomicAdd(&E.flags[FLAG_ACTIVE], act);
}


// ---- packed example block (bz_abi.h): the rows of the FINISHED games only, compacted in (round, slot, ply) order
// behind a 256-byte header -- what the iteration-end all-gather ships.  Two launches: a one-workgroup scan of the
// games' row counts (first row of every finished game -> pack_off), then one wave per game copies its rows.
struct PackedHdr {
    u64 magic, n_rows, n_games, cap_rows, na, game, dropped_rows, bytes;
    u64 offs[8];  // own, opp, pi, game id, z, mover, act, ply: byte offsets from the start of the block
    u64 pad[16];
};
static_assert(sizeof(PackedHdr) == 256, "packed example header");
constexpr u64 kPackedMagic = 0x425A50414B000001ULL;  // "BZPAK" + layout version 1
struct PackedLayout { int64_t offs[8]; int64_t total; };

__global__ void __launch_bounds__(1024) k_pack_scan(EngineDev E, PackedHdr* hdr, PackedLayout L, u64 cap, int append, int game) {
    __shared__ u32 wsum[16];
    __shared__ u32 s_games, s_rows_end;
    const int n = E.rounds * E.B, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool bad = false;
    u32 carry = 0, games0 = 0;
    u64 dropped0 = 0;
    if (append) {  // every thread reads the header before thread 0 rewrites it (barriers below)
        // (~0 in dropped_rows is final for a block: the header a bad append rewrote would otherwise match the next call)
        bad = hdr->magic != kPackedMagic || hdr->cap_rows != cap || hdr->na != (u64)E.na || hdr->bytes != (u64)L.total ||
              hdr->game != (u64)game || hdr->dropped_rows == ~0ULL;
        carry = (u32)hdr->n_rows; games0 = (u32)hdr->n_games; dropped0 = hdr->dropped_rows;
    }
    if (threadIdx.x == 0) { s_games = 0; s_rows_end = carry; }
    __syncthreads();
    u32 total_all = carry;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int i = c0 + (int)threadIdx.x;
        const int len = i < n ? E.ex_len[i] : -1;
        const u32 v = len > 0 ? (u32)len : 0u;
        u32 x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const u32 y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        u32 woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const u32 sw = wsum[w]; tot += sw; if (w < wave) woff += sw; }
        const u32 first = total_all + woff + x - v;
        if (i < n) {
            const bool fits = len >= 0 && !bad && (u64)first + v <= cap;
            E.pack_off[i] = fits ? (int32_t)first : -1;
            if (fits) { atomicAdd(&s_games, 1u); atomicMax(&s_rows_end, first + v); }
        }
        total_all += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        hdr->magic = kPackedMagic; hdr->cap_rows = cap; hdr->na = (u64)E.na; hdr->bytes = (u64)L.total;
        hdr->game = (u64)game;
        for (int k = 0; k < 8; ++k) hdr->offs[k] = (u64)L.offs[k];
        if (!bad) { hdr->n_rows = s_rows_end; hdr->n_games = games0 + s_games; }  // a bad append keeps both words as they are
        hdr->dropped_rows = bad ? ~0ULL : dropped0 + (u64)(total_all - s_rows_end);
    }
}

__global__ void __launch_bounds__(256) k_pack_rows(EngineDev E, char* blk, PackedLayout L) {
    const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= E.rounds * E.B) return;
    const int off = E.pack_off[i];
    if (off < 0) return;
    const int len = E.ex_len[i], round = i / E.B, g = i - round * E.B;
    const size_t src = (size_t)i * E.t_max;  // [round][slot][ply]
    u64* own = reinterpret_cast<u64*>(blk + L.offs[0]) + off; u64* opp = reinterpret_cast<u64*>(blk + L.offs[1]) + off;
    float* pi = reinterpret_cast<float*>(blk + L.offs[2]) + (size_t)off * E.na;
    int64_t* gid = reinterpret_cast<int64_t*>(blk + L.offs[3]) + off;
    int8_t* z = reinterpret_cast<int8_t*>(blk + L.offs[4]) + off; int8_t* mv = reinterpret_cast<int8_t*>(blk + L.offs[5]) + off;
    uint8_t* act = reinterpret_cast<uint8_t*>(blk + L.offs[6]) + off; uint8_t* ply = reinterpret_cast<uint8_t*>(blk + L.offs[7]) + off;
    const int64_t id = (int64_t)(E.id_base + (u64)round * E.id_stride + (u64)g);
    for (int t = lane; t < len; t += 64) {
        own[t] = E.ex_own[src + t]; opp[t] = E.ex_opp[src + t]; gid[t] = id; z[t] = E.ex_z[src + t];
        mv[t] = E.ex_mover[src + t]; act[t] = E.ex_act[src + t]; ply[t] = (uint8_t)t;
    }
    const float* sp = E.ex_pi + src * E.na;  // a game's rows are consecutive at both ends: one straight copy
    for (int k = lane; k < len * E.na; k += 64) pi[k] = sp[k];
}

// ---- policy surprise weighting: one-lane-per-game kernels around the search and the play kernels
// the raw priors of every active game's expanded root -- fresh or kept from the previous move -- before k_root_noise /
// k_cap_noise rewrite them (bz_engine_root_noise); without noise nothing rewrites them and bz_engine_play launches this
template <class G>
__global__ void __launch_bounds__(256) k_surp_save(EngineDev E, SurpDev S) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B || E.g_state[g] != 0) return;
    const Node r = E.nodes[(size_t)g * E.ncap];
    const int n = (int)(r.info & 0xFFu);
    const Edge* ed = E.edges + (size_t)g * E.ecap + r.edge0;
    float* pr = S.prior + (size_t)g * G::MAXCH;
    for (int i = 0; i < n && i < G::MAXCH; ++i) pr[i] = ed[i].P;
}
// in front of the play kernel: the row it is about to write, by its own rule (budget: the playout cap's, or null -- a fast
// search records nothing)
// (the row rule, shared with k_root_q, DESIGN.md 3.18: an active slot with room for a row whose search had the full budget;
// 1 + the row's index into the [rounds][B][t_max] example arrays, 0: this play records nothing)
__device__ __forceinline__ u64 dev_pending_row(const EngineDev& E, int g, const u32* budget) {
    const int nex = E.g_state[g] == 0 ? E.g_nex[g] : E.t_max;
    if (nex < E.t_max && !(budget && budget[g] < (u32)E.sims))
        return ((u64)E.g_round[g] * (u64)E.B + (u64)g) * (u64)E.t_max + (u64)nex + 1ULL;
    return 0;
}
__global__ void __launch_bounds__(256) k_surp_note(EngineDev E, SurpDev S, const u32* budget) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B) return;
    S.pend[g] = dev_pending_row(E, g, budget);
}
// behind it: the noted row's kl from the pi the play kernel recorded and the saved priors (the searched tree is still in
// place: the root's edges give the actions)
template <class G>
__global__ void __launch_bounds__(256) k_surp_kl(EngineDev E, SurpDev S) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B) return;
    const u64 p = S.pend[g];
    if (p == 0) return;
    S.pend[g] = 0;
    const size_t row = (size_t)(p - 1ULL);
    const Node r = E.nodes[(size_t)g * E.ncap];
    int n = (int)(r.info & 0xFFu);
    n = n < G::MAXCH ? n : G::MAXCH;
    const Edge* ed = E.edges + (size_t)g * E.ecap + r.edge0;
    const float* pi = E.ex_pi + row * G::NA;
    const float* pr = S.prior + (size_t)g * G::MAXCH;
    S.ex_kl[row] = surprise_kl(n, [pi, ed](int i) { return pi[e_action(ed[i].w0)]; }, [pr](int i) { return pr[i]; });
}
// THE walk of the kernels that put a per-row array into the packed block's row order, over the pack_off k_pack_scan left (it
// counts the rows earlier engines appended): one wave per game i of [rounds, B], the game's rows 64 at a time; row(i, src, dst)
// with src the row's index in the engine's [rounds, B, t_max] arrays and dst < cap its row in the block
template <class Row>
__device__ __forceinline__ void dev_pack_walk(const EngineDev& E, int64_t cap, Row row) {
    const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= E.rounds * E.B) return;
    const int off = E.pack_off[i];
    if (off < 0) return;
    const int len = E.ex_len[i];
    const size_t src = (size_t)i * E.t_max;
    for (int t = lane; t < len && t < E.t_max && (int64_t)off + t < cap; t += 64) row(i, src + t, (size_t)off + t);
}
// a float per row -- ex_kl, ex_q -- in the packed block's row order
__global__ void __launch_bounds__(256) k_pack_f32(EngineDev E, const float* src, float* out, int64_t cap) {
    dev_pack_walk(E, cap, [=](int, size_t s, size_t d) { out[d] = src[s]; });
}

// ---- search-value targets: in front of the play kernel, while the searched tree is in place -- the row the
// play is about to write gets the root's search value from the raw visit statistics (whatever the play kernel records as pi:
// Gumbel's improved policy, the pruned visits of forced playouts), one lane per game
__global__ void __launch_bounds__(256) k_root_q(EngineDev E, ValueDev V, const u32* budget) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B) return;
    const u64 p = dev_pending_row(E, g, budget);
    if (p == 0) return;
    const Node r = E.nodes[(size_t)g * E.ncap];
    const Edge* ed = E.edges + (size_t)g * E.ecap + r.edge0;
    V.ex_q[(size_t)(p - 1ULL)] = root_value((int)(r.info & 0xFFu), [ed](int i) { return e_N(ed[i].w0); }, [ed](int i) { return ed[i].W; });
}

// ---- ownership targets: in front of the play kernel, behind k_root_policy / k_forced_root_policy, which left
// the action the play kernel is about to play in O.act (the same choice by the same functions).  One lane per
// game applies it to the root, repeats dev_play_tail's terminal test and stores a finished game's final board in absolute
// colours.  The play kernel's own refusal (a row to record and no room for it) is repeated too: such a game is not finished.
// (budget: the playout cap's, or null -- a fast search records no row, and finishes its game all the same)
template <class G>
__global__ void __launch_bounds__(256) k_own_final(EngineDev E, OwnDev O, const u32* budget) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B || E.g_state[g] != 0) return;
    const int a = O.act[g];
    if (a < 0 || a >= G::NA) return;  // (no search has expanded this slot's root)
    const bool record = !(budget && budget[g] < (u32)E.sims);
    if (record && E.g_nex[g] >= E.t_max) return;
    const int round = E.g_round[g];
    if (round < 0 || round >= E.rounds) return;
    const Node root = E.nodes[(size_t)g * E.ncap];
    u64 own, opp;
    G::apply(root.own, root.opp, a, &own, &opp);
    const int tm = -(int)E.g_to_move[g];
    const u64 lg = G::legal(own, opp);
    int tv;
    if (!G::terminal(own, opp, tm, lg, &tv)) return;
    const size_t i = (size_t)round * E.B + g;
    O.fin_x[i] = tm == 1 ? own : opp;
    O.fin_o[i] = tm == 1 ? opp : own;
}
// ---- resignation: one lane per game around the play kernel.  k_resign_note, the first launch of
// bz_engine_play: the root value of the search that has just ended (k_root_q's expression on the same raw statistics) goes
// through the mover's streak (a full search only: budget is the playout cap's, or null); the first fire of a game is recorded;
// a game that is not played out ends there -- no row, no move, the other side wins, z back-filled over the rows so far as
// dev_play_tail does at a terminal position -- and its slot leaves g_state == 0, so that every kernel up to k_resign_finish
// skips it and dev_pending_row answers 0 for it.
template <class G>
__global__ void __launch_bounds__(256) k_resign_note(EngineDev E, ResignDev R, const u32* budget) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B || E.g_state[g] != 0) return;
    const int round = E.g_round[g];
    if (round < 0 || round >= E.rounds) return;
    const size_t i = (size_t)round * E.B + g;
    const bool out = resign_played_out(E.seed, E.id_base + (u64)round * E.id_stride + (u64)g, R.playout_q);
    R.played_out[i] = out ? 1 : 0;
    if (budget && budget[g] < (u32)E.sims) return;  // a fast search: the threshold is calibrated on full ones
    const Node r = E.nodes[(size_t)g * E.ncap];
    const int n = (int)(r.info & 0xFFu);
    if (n == 0) return;  // (no search has expanded this slot's root)
    const Edge* ed = E.edges + (size_t)g * E.ecap + r.edge0;
    const float q = root_value(n, [ed](int k) { return e_N(ed[k].w0); }, [ed](int k) { return ed[k].W; });
    const int tm = E.g_to_move[g];
    uint8_t* st = R.streak + i * 2 + (tm == 1 ? 0 : 1);
    int s;
    const bool fire = resign_step(q, R.threshold, R.consecutive, (int)*st, &s);
    *st = (uint8_t)s;
    if (!fire) return;
    if (R.side[i] == 0) { R.side[i] = (int8_t)tm; R.move[i] = E.g_moves[g]; R.q[i] = q; }
    if (out) return;
    const int nex = E.g_nex[g] < E.t_max ? E.g_nex[g] : E.t_max, w = -tm;
    const size_t rowbase = i * E.t_max;
    for (int t = 0; t < nex; ++t) E.ex_z[rowbase + t] = (int8_t)(w * E.ex_mover[rowbase + t]);
    E.ex_len[i] = nex;
    E.ex_winner[i] = (int8_t)w;
    atomicAdd(&E.flags[FLAG_FINISHED], 1u);
    E.g_state[g] = kStateResigned;
}
// behind the play kernel and k_surp_kl: a resigned slot starts its next game (restart and a round left) or stays finished.
// (Not in k_resign_note: the play kernel would play the fresh game's first move from the tree of the resigned one.)
template <class G>
__global__ void __launch_bounds__(256) k_resign_finish(EngineDev E, int restart) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.B || E.g_state[g] != kStateResigned) return;
    const int round = E.g_round[g];
    if (restart && round + 1 < E.rounds) { dev_start_game<G>(E, g, round + 1); return; }
    E.g_state[g] = 1;
}

// the rows' target boards in the packed block's row order (dev_pack_walk): every row of a game gets its game's final board in
// the row's own side-to-move frame
__global__ void __launch_bounds__(256) k_pack_own(EngineDev E, OwnDev O, u64* fown, u64* fopp, int64_t cap) {
    dev_pack_walk(E, cap, [=](int i, size_t s, size_t d) {
        u64 a, b;
        ownership_row(O.fin_x[i], O.fin_o[i], (int)E.ex_mover[s], &a, &b);
        fown[d] = a; fopp[d] = b;
    });
}

// ---- the root store (S = 0: off), set by bz_engine_set_root_store in the caller's buffer: finished searches of
// roots at most D - 1 plies behind a game's start, keyed by the root's position, S entries behind an open-addressed index of
// n_idx >= 2 S words (entry + 1; 0 = empty).  An entry is one slot's arena image -- nodes, edges, node_v and the slot's table
// entries of that search -- and every index inside it (edge0, child ids, the table's node ids) is relative to the slot's own
// region, so an image moves between slots and the store by plain copies.  k_store_save files the trees of a finished search,
// k_store_seed lays a stored tree of a slot's next root where k_root_begin takes the slot's previous tree from: the carry-over
// then does what it does with a slot's own previous search.  A kernel argument of these two kernels only.
struct __attribute__((aligned(64))) StoreHdr { u64 own, opp, epoch; u32 n_nodes, n_edges, ready, pad[7]; };
static_assert(sizeof(StoreHdr) == 64, "layout");
struct StoreDev {
    int S, D, n_idx, base;  // base: the plies a game starts with (the fixed two-ply openings)
    u32* n_used;            // entries claimed so far
    u32* idx;               // [n_idx]
    StoreHdr* hdr;          // [S]
    u32* mark;              // [B]: the generation a slot was last seeded under (what its search then sees as the previous one)
    Node* nodes; Edge* edges; float* node_v; u64* tt;  // [S][ncap], [S][ecap], [S][ncap], [S][tt_buckets * 16]
};
constexpr int kCntSeededEvals = 11, kCntSeededSearches = 12, kCntStoreSaves = 13;  // counters[] words, written like kCntCollisions
constexpr int kCntReplaySeeds = 14, kCntReplaySims = 15;  // the replay seed's: searches it seeded, simulations they came with

__device__ __forceinline__ u32 store_home(const StoreDev& St, u64 own, u64 opp) { return (u32)(hash_pos(own, opp) >> 20) & (u32)(St.n_idx - 1); }
// the entry holding (own, opp) under `epoch`, or -1; *at: the index word the probe stopped at (an empty one on a miss)
__device__ __forceinline__ int store_find(const StoreDev& St, u64 own, u64 opp, u64 epoch, u32* at) {
    u32 p = store_home(St, own, opp);
    for (int k = 0; k < St.n_idx; ++k, p = (p + 1u) & (u32)(St.n_idx - 1)) {
        const u32 w = St.idx[p];
        if (w == 0u || w > (u32)St.S) { *at = p; return -1; }
        const StoreHdr& h = St.hdr[w - 1u];
        if (h.own == own && h.opp == opp && h.epoch == epoch) { *at = p; return (int)(w - 1u); }
    }
    *at = ~0u;
    return -1;
}
__device__ __forceinline__ bool store_depth_ok(const EngineDev& E, const StoreDev& St, int g) {
    const int d = E.g_moves[g] - St.base;
    return E.g_state[g] == 0 && d >= 0 && d < St.D;
}
__device__ __forceinline__ u32 tt_gen_before(u32 gen) { return gen == 1u ? kTtGenMax - 1u : gen - 1u; }

// what tt_lookup_insert answered when node `i` of slot g's finished search was created: true iff it took its evaluation from
// the previous search's arena.  The table only ever gains entries during a search (free slots are filled, live ones stay), and
// an entry's node id says when: the entries below i are the table that lookup saw.
__device__ __forceinline__ bool tt_replay_from_prev(const EngineDev& E, int g, u32 i, u32 gen, u32 prev_nodes) {
    const Node nd = E.nodes[(size_t)g * E.ncap + i];
    if (nd.info & kTerm) return false;  // (terminal children are never looked up)
#ifdef BZ_EXP_TT_WEAK_HASH
    const u64 h = hash_pos(nd.own, nd.opp) & 1u;
#else
    const u64 h = hash_pos(nd.own, nd.opp);
#endif
    const u32 tag = (u32)(h >> 32), gen_prev = tt_gen_before(gen);
    const u64* bucket = E.tt + ((size_t)g * (size_t)E.tt_buckets + (size_t)(h & (u64)(E.tt_buckets - 1))) * 16;
    u32 hit = ~0u;
    for (int s = 0; s < 16; ++s) {
        const u64 e = bucket[s];
        const u32 meta = (u32)(e >> 32), egen = meta >> kChildBits;
        const bool cur = egen == gen && (meta & kChildMask) < i, prv = prev_nodes != 0u && egen == gen_prev;
        if ((cur || prv) && (u32)e == tag) {
            const u32 key = ((prv ? 1u : 0u) << 20) | ((u32)s << 16) | (meta & kChildMask);
            hit = key < hit ? key : hit;
        }
    }
    if (hit == ~0u || (hit >> 20) == 0u) return false;
    const u32 x = hit & kChildMask;
    if (x == 0u || x >= prev_nodes) return false;
    const Node xn = E.nodes_alt[(size_t)g * E.ncap + x];
    return xn.own == nd.own && xn.opp == nd.opp && !(xn.info & kTerm) && (xn.info & 0xFFu) != 0u;
}

// Behind the last tree step of search `gen`, in front of the play kernel.  Blocks 0 .. B - 1: slot b, if this search was seeded
// for it, counts the evaluations it took from the seeded tree (counters[11]).  Block B files the finished trees: slots in
// ascending order, 256 at a time -- every lane looks its slot's root up, lane 0 then claims entries for the roots still
// missing (first come = lowest slot: which tree a root gets does not depend on timing), and the block copies them in.  A full
// store files nothing more.  budget: the playout cap's, or null -- a fast search's small tree is not worth an entry.
__global__ void __launch_bounds__(256) k_store_save(EngineDev E, StoreDev St, u32 gen, u64 epoch, const u32* budget) {
    __shared__ int claim[256];
    __shared__ u32 part[256];
    const int t = threadIdx.x;
    if ((int)blockIdx.x < E.B) {
        const int g = blockIdx.x;
        const GameHot& hot = E.hot[g];
        if (E.g_state[g] != 0 || hot.tt_gen != gen || hot.last_gen != gen || hot.prev_nodes == 0u || St.mark[g] != tt_gen_before(gen)) return;
        const u32 n = hot.n_nodes < (u32)E.ncap ? hot.n_nodes : (u32)E.ncap;
        u32 mine = 0;
        for (u32 i = 1u + (u32)t; i < n; i += 256u) mine += tt_replay_from_prev(E, g, i, gen, hot.prev_nodes) ? 1u : 0u;
        part[t] = mine;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (t < o) part[t] += part[t + o]; __syncthreads(); }
        if (t == 0 && part[0]) atomicAdd(reinterpret_cast<unsigned long long*>(E.counters) + kCntSeededEvals, (unsigned long long)part[0]);
        return;
    }
    const size_t ttn = (size_t)E.tt_buckets * 16;
    for (int g0 = 0; g0 < E.B; g0 += 256) {
        const int g = g0 + t;
        int c = -1;  // -2: a root to file
        if (g < E.B && store_depth_ok(E, St, g) && E.hot[g].last_gen == gen && E.hot[g].tt_gen == gen && E.hot[g].n_nodes > 1u &&
            E.hot[g].n_nodes <= (u32)E.ncap && E.hot[g].n_edges <= (u32)E.ecap && !(budget && budget[g] < (u32)E.sims)) {
            const Node r = E.nodes[(size_t)g * E.ncap];
            u32 at;
            if (store_find(St, r.own, r.opp, epoch, &at) < 0) c = -2;
        }
        claim[t] = c;
        __syncthreads();
        if (t == 0) {
            for (int j = 0; j < 256; ++j) {
                if (claim[j] != -2) continue;
                claim[j] = -1;
                const u32 used = *St.n_used;
                if (used >= (u32)St.S) continue;
                const int gj = g0 + j;
                const Node r = E.nodes[(size_t)gj * E.ncap];
                u32 at;
                if (store_find(St, r.own, r.opp, epoch, &at) >= 0 || at == ~0u) continue;  // (a lower slot of this launch filed this root)
                StoreHdr h{};
                h.own = r.own; h.opp = r.opp; h.epoch = epoch; h.n_nodes = E.hot[gj].n_nodes; h.n_edges = E.hot[gj].n_edges; h.ready = 0u;
                St.hdr[used] = h;
                St.idx[at] = used + 1u;
                *St.n_used = used + 1u;
                __threadfence();
                claim[j] = (int)used;
            }
        }
        __syncthreads();
        for (int j = 0; j < 256; ++j) {
            const int en = claim[j];
            if (en < 0) continue;
            const int gj = g0 + j;
            const u32 nn = St.hdr[en].n_nodes, ne = St.hdr[en].n_edges;
            const uint4* sn = reinterpret_cast<const uint4*>(E.nodes + (size_t)gj * E.ncap);
            uint4* dn = reinterpret_cast<uint4*>(St.nodes + (size_t)en * E.ncap);
            for (u32 k = t; k < nn * 2u; k += 256u) dn[k] = sn[k];
            const uint4* se = reinterpret_cast<const uint4*>(E.edges + (size_t)gj * E.ecap);
            uint4* de = reinterpret_cast<uint4*>(St.edges + (size_t)en * E.ecap);
            for (u32 k = t; k < ne; k += 256u) de[k] = se[k];
            const float* sv = E.node_v + (size_t)gj * E.ncap;
            float* dv = St.node_v + (size_t)en * E.ncap;
            for (u32 k = t; k < nn; k += 256u) dv[k] = sv[k];
            const u64* st = E.tt + (size_t)gj * ttn;
            u64* dt = St.tt + (size_t)en * ttn;
            for (size_t k = t; k < ttn; k += 256) {  // this search's entries only; the rest of the image is empty
                const u64 e = st[k];
                dt[k] = ((u32)(e >> 32) >> kChildBits) == gen ? e : 0ULL;
            }
        }
        __syncthreads();
        if (t == 0)
            for (int j = 0; j < 256; ++j)
                if (claim[j] >= 0) {
                    St.hdr[claim[j]].ready = 1u;
                    atomicAdd(reinterpret_cast<unsigned long long*>(E.counters) + kCntStoreSaves, 1ULL);
                }
        __syncthreads();
    }
}

// In front of k_root_begin, on the arena the search of generation `gen` just ran in -- the one the host is about to make the
// previous one.  Block g: if slot g's next root is stored, the entry replaces the slot's tree there, its table entries take
// generation `gen`, and the slot's n_nodes / last_gen say "my previous search, `gen`, left n_nodes nodes": k_root_begin and
// tt_lookup_insert read nothing else.  The slot's table holds nothing but the image afterwards (its older entries would be
// dead from the next search on anyway).
__global__ void __launch_bounds__(256) k_store_seed(EngineDev E, StoreDev St, u32 gen, u64 epoch) {
    __shared__ int found;
    const int g = blockIdx.x, t = threadIdx.x;
    if (t == 0) {
        int en = -1;
        if (store_depth_ok(E, St, g)) {
            u32 at;
            en = store_find(St, E.g_own[g], E.g_opp[g], epoch, &at);
            if (en >= 0 && (St.hdr[en].ready == 0u || St.hdr[en].n_nodes > (u32)E.ncap || St.hdr[en].n_edges > (u32)E.ecap)) en = -1;
        }
        found = en;
    }
    __syncthreads();
    const int en = found;
    if (en < 0) return;
    const u32 nn = St.hdr[en].n_nodes, ne = St.hdr[en].n_edges;
    const uint4* sn = reinterpret_cast<const uint4*>(St.nodes + (size_t)en * E.ncap);
    uint4* dn = reinterpret_cast<uint4*>(E.nodes + (size_t)g * E.ncap);
    for (u32 k = t; k < nn * 2u; k += 256u) dn[k] = sn[k];
    const uint4* se = reinterpret_cast<const uint4*>(St.edges + (size_t)en * E.ecap);
    uint4* de = reinterpret_cast<uint4*>(E.edges + (size_t)g * E.ecap);
    for (u32 k = t; k < ne; k += 256u) de[k] = se[k];
    const float* sv = St.node_v + (size_t)en * E.ncap;
    float* dv = E.node_v + (size_t)g * E.ncap;
    for (u32 k = t; k < nn; k += 256u) dv[k] = sv[k];
    const size_t ttn = (size_t)E.tt_buckets * 16;
    const u64* st = St.tt + (size_t)en * ttn;
    u64* dt = E.tt + (size_t)g * ttn;
    for (size_t k = t; k < ttn; k += 256) {
        const u64 e = st[k];
        dt[k] = e ? ((e & 0xFFFFFFFFULL) | ((u64)((gen << kChildBits) | ((u32)(e >> 32) & kChildMask)) << 32)) : 0ULL;
    }
    if (t == 0) {
        E.hot[g].n_nodes = nn; E.hot[g].last_gen = gen;
        St.mark[g] = gen;
        atomicAdd(reinterpret_cast<unsigned long long*>(E.counters) + kCntSeededSearches, 1ULL);
    }
}

// ---- The replay seed.  A fresh search from the child the slot just played re-creates that child's old subtree
// node for node -- deterministic PUCT on evaluations the carry-over hands back -- for the first N_e - 1 simulations, N_e the
// visits of the edge into it.  Behind k_root_begin, block g (one lane group) copies that subtree from the previous arena into
// the new tree instead: nodes and edge blocks compacted in their old creation order (the order the replay would create and
// expand them in), N / W / P / node_v as they stand, child links rewritten; then it replays the evaluation cache's part --
// tt_lookup_insert for every copied non-terminal node in creation order, the very calls the replay makes -- so that the table,
// n_nodes, n_edges and the work counters are what N_e - 1 simulations would have left.  The slot then has seeded = N_e - 1.
// Nothing is seeded -- the search runs as it always did -- when the new root is not found behind an edge of the old root (a
// restarted slot, other roots), when the carry-over is refused or the previous arena holds a tree the root store put there, when
// the previous search was not a plain one (do_seed = 0), or when a lookup of the replay would have missed (a full bucket): the
// replay would have sent that leaf through the net, which a copy cannot; the table entries written so far are taken out again.
// LDS, per node of the previous tree: {new id 13 | new first edge 19} (first: its edge count), its parent, and the old id by new id.
template <class G>
__global__ void __launch_bounds__(G::GW) k_replay_seed(EngineDev E, u32 gen, int do_seed, const u32* store_mark) {
    constexpr int kGW = G::GW;
    constexpr u32 kNone = 0xFFFFu;
    extern __shared__ u32 s_map[];
    uint16_t* s_par = reinterpret_cast<uint16_t*>(s_map + E.ncap);
    uint16_t* s_ord = s_par + E.ncap;
    const int g = blockIdx.x, sub = threadIdx.x;
    GameHot* hot = E.hot + g;
    const bool searching = E.g_state[g] == 0 && E.leaf_kind[g] == LEAF_EVAL;
    const u32 pn = hot->prev_nodes;
    u32 cand = ~0u;  // (visits of the edge into it << 13) | the previous tree's node that holds the new root's position
    const Node* sn = E.nodes_alt + (size_t)g * E.ncap;
    const Edge* se = E.edges_alt + (size_t)g * E.ecap;
    if (do_seed && searching && pn > 1u && pn <= (u32)E.ncap && !(store_mark && store_mark[g] == tt_gen_before(gen))) {
        const u64 rown = E.g_own[g], ropp = E.g_opp[g];
        const Node oroot = sn[0];
        const u32 n0 = ((oroot.info & kTerm) || oroot.edge0 + (oroot.info & 0xFFu) > (u32)E.ecap) ? 0u : (oroot.info & 0xFFu);
        for (u32 i = sub; i < n0; i += kGW) {
            const Edge e = se[oroot.edge0 + i];
            u32 ch = e_child(e.w3), N = e_N(e.w0);
            if (!ch || ch >= pn || e_decided(e.w0)) continue;
            const Node* cn = sn + ch;
            if (cn->legal == 0 && (cn->info & 0xFFu) == 1u && cn->edge0 < (u32)E.ecap) {  // the driver skips a forced pass: the root lies behind the pass edge
                const Edge pe = se[cn->edge0];
                ch = e_child(pe.w3); N = e_N(pe.w0);
                if (!ch || ch >= pn || e_decided(pe.w0)) continue;
                cn = sn + ch;
            }
            const u32 ci = cn->info;
            if (cn->own == rown && cn->opp == ropp && !(ci & kTerm) && (ci & 0xFFu) != 0u && N >= 2u) cand = ch | (N << kChildBits);
        }
    }
    cand = group_min_u32<kGW>(cand);
    if (cand == ~0u) {  // (the same in every lane)
        if (sub == 0) hot->seeded = searching ? 0u : kPaceIdle;
        return;
    }
    const u32 r_old = cand & kChildMask, seeded = (cand >> kChildBits) - 1u;
    // ---- every node's edge count and parent, lanes over the nodes behind r_old (a child is younger than its parent)
    for (u32 i = r_old + sub; i < pn; i += kGW) s_par[i] = (uint16_t)kNone;
    __syncthreads();
    for (u32 i = r_old + sub; i < pn; i += kGW) {
        const Node nd = sn[i];
        const u32 n = ((nd.info & kTerm) || nd.edge0 + (nd.info & 0xFFu) > (u32)E.ecap) ? 0u : (nd.info & 0xFFu);
        s_map[i] = n;
        for (u32 j = 0; j < n; ++j) {
            const u32 ch = e_child(se[nd.edge0 + j].w3);
            if (ch > i && ch < pn) s_par[ch] = (uint16_t)i;
        }
    }
    __syncthreads();
    // ---- the subtree in creation order: new ids and first edges (every lane runs the same sweep on the same words)
    u32 nT = 0, eT = 0;
    for (u32 i = r_old; i < pn; ++i) {
        const u32 p = s_par[i], n = s_map[i];
        const bool in = i == r_old || (p != kNone && s_map[p] != ~0u);
        if (in) {
            s_map[i] = nT | (eT << kChildBits);
            s_ord[nT] = (uint16_t)i;
            ++nT; eT += n;
        } else {
            s_map[i] = ~0u;
        }
    }
    __syncthreads();
    if (eT > (u32)E.ecap) {  // (never, for a tree a search built: the subtree's edges are a subset of the old tree's)
        if (sub == 0) hot->seeded = 0u;
        return;
    }
    // ---- the copy, lanes over the nodes; what the replay's walks would have counted, from N and the child counts
    Node* dn = E.nodes + (size_t)g * E.ncap;
    Edge* de = E.edges + (size_t)g * E.ecap;
    const float* sv = E.node_v_alt + (size_t)g * E.ncap;
    float* dv = E.node_v + (size_t)g * E.ncap;
    u32 c_vis = 0, c_scored = 0, c_exp = 0, c_written = 0, root_sum = 0;
    for (u32 k = sub; k < nT; k += kGW) {
        const u32 i = s_ord[k];
        const Node nd = sn[i];
        const u32 e0n = s_map[i] >> kChildBits;
        const u32 n = ((nd.info & kTerm) || nd.edge0 + (nd.info & 0xFFu) > (u32)E.ecap) ? 0u : (nd.info & 0xFFu);  // (as counted above)
        u32 sumN = 0;
        for (u32 j = 0; j < n; ++j) {
            Edge e = se[nd.edge0 + j];
            const u32 ch = e_child(e.w3);
            if (ch) {  // (first edge: only an expanded child's edge word has one)
                const u32 mc = ch < pn ? s_map[ch] : 0u;
                e.w3 = e_nch(e.w0) ? mc : (mc & kChildMask);
            }
            sumN += e_N(e.w0);
            de[e0n + j] = e;
        }
        dv[k] = sv[i];
        if (k != 0u) {
            Node out;
            out.own = nd.own; out.opp = nd.opp; out.legal = nd.legal; out.edge0 = n ? e0n : 0u; out.info = nd.info;
            dn[k] = out;
        } else {
            root_sum = sumN;
        }
        c_vis += sumN; c_scored += n * sumN; c_exp += n ? 1u : 0u; c_written += n;
    }
    root_sum = group_sum_u32<kGW>(root_sum);
    group_fence();  // the nodes written above are what the lookups below confirm this search's entries against
    // ---- the evaluation cache's part of the replay: one lookup per created non-terminal node, in creation order
    u32 hits = 0, hits_prev = 0;
    bool exact = root_sum == seeded;
    for (u32 k = 1; exact && k < nT; ++k) {
        const Node nd = sn[s_ord[k]];  // (one address for the whole group)
        if (nd.info & kTerm) continue;
        u32 src = 0, src_e0 = 0;
        if (tt_lookup_insert<kGW>(E, g, sub, nd.own, nd.opp, gen, pn, k, src, src_e0)) { ++hits; hits_prev += (src & kSrcPrev) ? 1u : 0u; }
        else exact = false;
    }
    if (!exact) {  // not a pure copy phase: no seed, and no trace of it in the table
        u64* tt = E.tt + (size_t)g * (size_t)E.tt_buckets * 16;
        for (u32 k = sub; k < (u32)E.tt_buckets * 16u; k += kGW)
            if (((u32)(tt[k] >> 32) >> kChildBits) == gen) tt[k] = 0ULL;
        if (sub == 0) hot->seeded = 0u;
        return;
    }
    c_vis = group_sum_u32<kGW>(c_vis); c_scored = group_sum_u32<kGW>(c_scored);
    c_exp = group_sum_u32<kGW>(c_exp); c_written = group_sum_u32<kGW>(c_written);
    if (sub == 0) {
        const u32 rn = sn[r_old].info & 0xFFu;  // (the rest of node 0 is k_root_begin's: the position, the legal mask, the mover)
        dn[0].edge0 = 0; dn[0].info = (dn[0].info & ~0xFFu) | rn;
        hot->n_nodes = nT; hot->n_edges = eT; hot->root_n = rn; hot->seeded = seeded;
        atomicAdd(reinterpret_cast<unsigned long long*>(E.counters) + kCntReplaySeeds, 1ULL);
        atomicAdd(reinterpret_cast<unsigned long long*>(E.counters) + kCntReplaySims, (unsigned long long)seeded);
    }
    // the work counters, into the slot's wave's row of the per-wave slots (lane k: counter k)
    u32 add = 0;
    switch (sub) {
    case CNT_SIMS: add = seeded; break;
    case CNT_PATH_NODES: add = seeded + c_vis; break;
    case CNT_CHILD_SCORED: add = c_scored; break;
    case CNT_EDGES_BACKED: add = c_vis; break;
    case CNT_EXPANDED: add = c_exp; break;
    case CNT_CHILD_WRITTEN: add = c_written; break;
    case CNT_ENV_STEPS: add = nT - 1u; break;
    case CNT_CACHE_HITS: add = hits; break;
    case CNT_CACHE_HITS_PREV: add = hits_prev; break;
    default: break;
    }
    if (add)
        __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(E.cnt_slots) + (size_t)(g % E.n_cnt_slots) * CNT_N + sub,
                               (unsigned long long)add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

// ---------------------------------------------------------------- host side
struct bz_engine {
    bz_engine_cfg cfg;
    bz_engine_layout lay;
    EngineDev dev;
    bz_net* net;
    bz_mlp* mlp;  // BZ_EVAL_MLP_* (bz_engine_set_mlp)
    int64_t bytes;
    int pack_parity;  // which NEVAL buffer the last root_begin / select packed into
    int ttt_gw;       // lanes per game of the TTT-specialised fused search (cfg.ttt_lanes; 0 = the generic any-game kernel)
    uint32_t search_seq;  // searches begun so far: the evaluation cache's generation (entries of earlier searches are dead)
    uint64_t eval_epoch;  // bz_net_epoch of the weights the previous search evaluated with (carry-over needs the same ones)
    // bz_engines_step: ring of blocking-sync events that bounds how far the host thread runs ahead of this engine's
    // stream (created on first use)
    hipEvent_t ahead[4];
    int n_ahead;
    GumbelDev gumbel;  // Gumbel root search (bz_engine_set_gumbel); gumbel.m = 0: off
    GumbelInDev gin;   // Gumbel interior selection (bz_engine_set_gumbel_interior); gin.node_v = nullptr: off
    CapDev cap;        // playout cap randomisation (bz_engine_set_playout_cap); cap.fast = 0: off
    ForcedDev forced;  // forced playouts (bz_engine_set_forced_playouts); forced.k = 0: off
    SurpDev surp;      // policy surprise weighting (bz_engine_set_surprise); surp.prior = nullptr: off
    FpuDev fpu;        // first-play urgency reduction (bz_engine_set_fpu); fpu.root_w = nullptr: off
    int fpu_done;      // ... simulations selected so far in the current search: what an expand-only step has backed up when it is done
    SolveDev solve;    // proven wins, losses and draws (bz_engine_set_solver); solve.root = nullptr: off
    int64_t solve_bytes;  // ... the bytes bz_engine_root_begin zeroes in its buffer
    StopDev stop;      // exact early stop (bz_engine_set_early_stop); stop.stop_at = nullptr: off
    int stop_host_exit;   // ... engines_run leaves the step loop once no slot of this engine walks any more
    uint32_t* stop_ring;  // ... pinned host words [4], one per run-ahead mark in flight: stop.walked as of that mark (created on first use)
    ValueDev value;    // search-value targets (bz_engine_set_search_value); value.ex_q = nullptr: off
    OwnDev own;        // ownership targets (bz_engine_set_ownership); own.fin_x = nullptr: off
    ResignDev resign;  // resignation (bz_engine_set_resign); resign.streak = nullptr: off
    int64_t resign_bytes;  // ... the bytes bz_engine_reset_games zeroes in its buffer
    StoreDev store;    // the root store (bz_engine_set_root_store); store.S = 0: off
    int64_t store_index_bytes;  // ... its front part (fill count, index, entry headers): zeroing it empties the store
    // hashed evaluation symmetry (bz_engine_set_eval_symmetry); on the engine, not on the net: two pipelines
    // and two match players share one bz_net
    int sym_on;
    uint64_t sym_seed;
    // the replay seed (bz_engine_set_replay_seed): the switch (0 off, 1 on, 2 = the default: on where the engine
    // has more than kPaceAutoSlots slots); whether the search under way is
    // paced (engines_run / bz_engine_search set it behind bz_engine_root_begin, which clears it: the step API is never paced);
    // whether the last search run to its end was a whole paced one -- the only trees the seed copies from -- and the same of the
    // search before the one bz_engine_root_begin has just begun (it moves the one word into the other: a search begun through the
    // step API leaves nothing to seed from)
    int replay_seed, paced, seed_from_prev, seed_src;
};

namespace {
struct Carver {
    int64_t off = 0;
    int64_t take(int64_t bytes) { int64_t o = off; off += (bytes + 255) & ~int64_t(255); return o; }
};

struct Offsets {
    int64_t nodes, edges, nodes_alt, edges_alt, g_reuse, g_own, g_opp, g_to_move, g_state, g_moves, g_nex, g_round, g_passes, hot,
        path, lrec, leaf_kind, leaf_own, leaf_opp, c_own, c_opp, logits, value, ex_own, ex_opp, ex_pi, ex_z, ex_mover,
        ex_act, ex_len, ex_winner, ex_meta, root_N, root_W, root_P, counters, cnt_slots, flags, pack_off, tt, node_v, node_v_alt, total;
    int n_cnt_slots;
    int ncap, ecap, na, maxd;
    int ecache, tt_buckets;
};
inline bool net_eval(int ek) { return ek == BZ_EVAL_NET_F32 || ek == BZ_EVAL_NET_BF16 || ek == BZ_EVAL_NET_FP8; }
inline bool mlp_eval(int ek) { return ek == BZ_EVAL_MLP_F32 || ek == BZ_EVAL_MLP_BF16; }

// nodes a game's arena holds: a fresh tree grows by one node per simulation; with subtree reuse a kept
// subtree + sims new nodes must fit
inline int64_t nodes_per_game(const bz_engine_cfg& c) { return ((c.flags & BZ_ENGINE_REUSE_SUBTREE) ? 4 : 1) * ((int64_t)c.sims + 2); }
// leaves per step: flag bits 8..12 hold K - 1
inline int leaves_per_step(const bz_engine_cfg& c) { return (int)((c.flags & BZ_ENGINE_LEAVES_MASK) >> BZ_ENGINE_LEAVES_SHIFT) + 1; }
constexpr uint32_t kFlagBits = (1u << 13) - 1u;  // flag bits 0..12; the leaves-per-step field is the highest

bool cfg_ok(const bz_engine_cfg* c) {
    if (c && (c->flags & ~kFlagBits)) return false;  // bits above the leaves-per-step field are reserved
    if (!(c && c->game >= BZ_GAME_TTT && c->game <= BZ_GAME_REVERSI4 && c->n_games > 0 && c->sims >= 1 &&
          c->eval_kind >= 0 && c->eval_kind <= BZ_EVAL_MLP_BF16 && (!mlp_eval(c->eval_kind) || c->game == BZ_GAME_TTT) &&
          c->rounds >= 1 &&
          c->t_max >= 1 && c->dirichlet_eps >= 0.0f && c->dirichlet_eps <= 1.0f &&
          (c->dirichlet_eps == 0.0f || (c->dirichlet_alpha > 0.0f && c->dirichlet_alpha <= 1.0f)) &&
          (c->ttt_lanes == -1 || c->ttt_lanes == 0 || c->ttt_lanes == 1 || c->ttt_lanes == 2 || c->ttt_lanes == 4 ||
           c->ttt_lanes == 8)))
        return false;
    // the packed edge record holds node ids in 13 bits and visit counts in 14 (BZ_ENGINE_MAX_SIMS in bz_abi.h)
    return nodes_per_game(*c) <= kMaxNodes;
}

Offsets carve(const bz_engine_cfg& c) {
    Offsets o{};
    bool ttt = c.game == BZ_GAME_TTT;
    o.na = ttt ? TicTacToe::NA : Reversi::NA;
    o.maxd = ttt ? TicTacToe::MAXD : Reversi::MAXD;
    const bool reuse = (c.flags & BZ_ENGINE_REUSE_SUBTREE) != 0;
    o.ncap = (int)nodes_per_game(c);
    o.ecap = o.ncap * (ttt ? TicTacToe::MAXCH : Reversi::MAXCH);
    int64_t B = c.n_games, R = c.rounds, T = c.t_max;
    const int64_t K = leaves_per_step(c);
    Carver k;
    o.nodes = k.take(B * o.ncap * (int64_t)sizeof(Node));
    o.edges = k.take(B * o.ecap * (int64_t)sizeof(Edge));
    // evaluation cache: net evaluators only (a synthetic evaluation costs less than the lookup), not with subtree reuse
    // (a kept subtree's nodes are not in the new search's table).  2 = with carry-over: a second arena, like subtree reuse
    // (and not with leaf-parallel search: K > 1)
    o.ecache = ((c.flags & BZ_ENGINE_EVAL_CACHE) && net_eval(c.eval_kind) && !reuse && K == 1) ? ((c.flags & BZ_ENGINE_EVAL_CACHE_CARRY) ? 2 : 1) : 0;
    const bool two = reuse || o.ecache == 2;
    o.nodes_alt = k.take(two ? B * o.ncap * (int64_t)sizeof(Node) : 0);
    o.edges_alt = k.take(two ? B * o.ecap * (int64_t)sizeof(Edge) : 0);
    o.g_reuse = k.take(reuse ? B * 4 : 0);
    o.g_own = k.take(B * 8); o.g_opp = k.take(B * 8); o.g_to_move = k.take(B); o.g_state = k.take(B);
    o.g_moves = k.take(B * 4); o.g_nex = k.take(B * 4); o.g_round = k.take(B * 4); o.g_passes = k.take(B * 4);
    o.hot = k.take(B * (int64_t)sizeof(GameHot));
    // leaf-parallel search: K paths and K leaf records per game, K*B leaf / evaluator rows (row g*K + j = walk j of game g)
    o.path = k.take((int64_t)o.maxd * K * B * (int64_t)sizeof(PathEnt));
    o.lrec = k.take(K > 1 ? K * B * (int64_t)sizeof(LeafRec) : 0);
    o.leaf_kind = k.take(K * B); o.leaf_own = k.take(K * B * 8); o.leaf_opp = k.take(K * B * 8);
    o.c_own = k.take(K * B * 8); o.c_opp = k.take(K * B * 8);
    o.logits = k.take(K * B * o.na * 4); o.value = k.take(K * B * 4);
    o.ex_own = k.take(R * B * T * 8); o.ex_opp = k.take(R * B * T * 8); o.ex_pi = k.take(R * B * T * o.na * 4);
    o.ex_z = k.take(R * B * T); o.ex_mover = k.take(R * B * T); o.ex_act = k.take(R * B * T);
    o.ex_len = k.take(R * B * 4); o.ex_winner = k.take(R * B);
    // ex_own .. ex_meta are consecutive: ONE byte range [ex_own, ex_meta + 256) is what the all-gather ships
    o.ex_meta = k.take(256);
    o.root_N = k.take(B * o.na * 4); o.root_W = k.take(B * o.na * 4); o.root_P = k.take(B * o.na * 4);
    o.counters = k.take(kCntWords * 8);
    o.n_cnt_slots = (int)((B * 16 + 63) / 64) + 4;  // one slot per wave of the widest (group) launch (<= 16 lanes per game)
    o.cnt_slots = k.take((int64_t)o.n_cnt_slots * CNT_N * 8);
    o.flags = k.take(FLAG_N * 4);
    // (tests/test_gpu_pack.py finds pack_off as the LAST array of a workspace without the evaluation cache -- the arrays below
    // are then empty -- and proves that before it writes there: an array carved behind it makes that probe fail, not scribble)
    o.pack_off = k.take(R * B * 4);
    // the table's buckets: a power of two, >= 2 slots per live node (with carry-over two searches' entries are live)
    o.tt_buckets = 16;
    while ((int64_t)o.tt_buckets * 16 < (o.ecache == 2 ? 4 : 2) * (int64_t)o.ncap) o.tt_buckets *= 2;
    o.tt = k.take(o.ecache ? B * o.tt_buckets * 16 * 8 : 0);
    o.node_v = k.take(o.ecache ? B * o.ncap * 4 : 0);
    o.node_v_alt = k.take(o.ecache == 2 ? B * o.ncap * 4 : 0);
    o.total = k.off;
    return o;
}

template <class T> T* at(void* base, int64_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
inline dim3 grid_of(int B) { return dim3((B + 255) / 256); }
inline dim3 grid_groups(int B, int gw) { return dim3(((size_t)B * gw + 255) / 256); }
}  // namespace

#define BZ_LAUNCH_ONE(G, KERNEL, grid, stream, ...) \
    hipLaunchKernelGGL(KERNEL<G>, grid, dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__)
#define BZ_DISPATCH_IMPL(e, KERNEL, GRIDFN, stream, ...)                                                        \
    do {                                                                                                        \
        switch ((e)->cfg.game) {                                                                                \
        case BZ_GAME_TTT: BZ_LAUNCH_ONE(TicTacToe, KERNEL, GRIDFN((e)->dev.B, TicTacToe::GW), stream, __VA_ARGS__); break; \
        case BZ_GAME_REVERSI6: BZ_LAUNCH_ONE(Reversi6, KERNEL, GRIDFN((e)->dev.B, Reversi6::GW), stream, __VA_ARGS__); break; \
        case BZ_GAME_REVERSI4: BZ_LAUNCH_ONE(Reversi4, KERNEL, GRIDFN((e)->dev.B, Reversi4::GW), stream, __VA_ARGS__); break; \
        default: BZ_LAUNCH_ONE(Reversi, KERNEL, GRIDFN((e)->dev.B, Reversi::GW), stream, __VA_ARGS__); break;      \
        }                                                                                                       \
        BZ_LAUNCH_CHECK(#KERNEL);                                                                               \
    } while (0)
inline dim3 grid_lane(int B, int) { return grid_of(B); }
// one lane per game / G::GW lanes per game
#define BZ_DISPATCH(e, KERNEL, stream, ...) BZ_DISPATCH_IMPL(e, KERNEL, grid_lane, stream, __VA_ARGS__)
#define BZ_DISPATCH_G(e, KERNEL, stream, ...) BZ_DISPATCH_IMPL(e, KERNEL, grid_groups, stream, __VA_ARGS__)

namespace {
const char* kBadCfg = "bad config (note: sims <= 8189, or <= 2045 with BZ_ENGINE_REUSE_SUBTREE -- the packed edge record, bz_abi.h)";
const char* kBadFlags = "bad config: cfg.flags has bits set above bit 12 (the leaves-per-step field BZ_ENGINE_LEAVES_MASK ends there)";
// the preface of every entry point that takes a config: false, and the message, for reserved flag bits or a bad config
bool cfg_guard(const char* fn, const bz_engine_cfg* cfg) {
    if (cfg && (cfg->flags & ~kFlagBits)) { set_error("%s: %s", fn, kBadFlags); return false; }
    if (!cfg_ok(cfg)) { set_error("%s: %s", fn, kBadCfg); return false; }
    return true;
}
// the preface of every setter that takes a caller-owned buffer: BZ_OK, or the message and BZ_EINVAL for a null or misaligned
// buffer, small_rc for one below `need` bytes
int32_t option_buffer(const char* fn, const void* buf, int64_t bytes, int64_t need, int32_t small_rc = BZ_ENOMEM) {
    if (!buf || (reinterpret_cast<uintptr_t>(buf) & 255)) { set_error("%s: the buffer must be non-null and 256-byte aligned", fn); return BZ_EINVAL; }
    if (bytes < need) { set_error("%s: buffer too small (%lld < %lld)", fn, (long long)bytes, (long long)need); return small_rc; }
    return BZ_OK;
}
// Whether a search option (BZ_OPT_*) is on: THE place that reads the config's option fields and the setters' state.
bool option_on(const bz_engine_cfg& c, int opt) {
    switch (opt) {
    case BZ_OPT_REUSE_SUBTREE: return (c.flags & BZ_ENGINE_REUSE_SUBTREE) != 0;
    case BZ_OPT_LEAVES: return leaves_per_step(c) > 1;
    case BZ_OPT_DIRICHLET: return c.dirichlet_eps > 0.0f;
    default: return false;  // (switched on by a setter: no config carries it)
    }
}
bool option_on(const bz_engine* e, int opt) {
    switch (opt) {
    case BZ_OPT_GUMBEL: return e->gumbel.m > 0;
    case BZ_OPT_GUMBEL_INTERIOR: return e->gin.node_v != nullptr;
    case BZ_OPT_PLAYOUT_CAP: return e->cap.fast > 0;
    case BZ_OPT_FORCED_PLAYOUTS: return e->forced.k > 0.0f;
    case BZ_OPT_FPU: return e->fpu.root_w != nullptr;
    case BZ_OPT_SOLVER: return e->solve.root != nullptr;
    case BZ_OPT_EARLY_STOP: return e->stop.stop_at != nullptr;
    case BZ_OPT_ROOT_STORE: return e->store.S > 0;
    case BZ_OPT_SURPRISE: return e->surp.prior != nullptr;
    case BZ_OPT_SEARCH_VALUE: return e->value.ex_q != nullptr;
    case BZ_OPT_OWNERSHIP: return e->own.fin_x != nullptr;
    case BZ_OPT_RESIGN: return e->resign.streak != nullptr;
    default: return option_on(e->cfg, opt);
    }
}
// the first option that is on in the engine (in a config: that the config carries) and does not run with `opt`: true and the message
bool option_refusal(const char* fn, int opt, const bz_engine* e) {
    return refuse_first_conflict(fn, opt, [e](int o) { return option_on(e, o); });
}
bool option_refusal(const char* fn, int opt, const bz_engine_cfg& c) {
    return refuse_first_conflict(fn, opt, [&c](int o) { return option_on(c, o); });
}
}  // namespace

BZ_EXPORT int32_t bz_option_conflict(int32_t a, int32_t b) { return option_id_ok(a) && option_id_ok(b) ? (option_conflict(a, b) ? 1 : 0) : -1; }
BZ_EXPORT const char* bz_option_name(int32_t a) { return option_id_ok(a) ? kOptions[a].phrase : nullptr; }

BZ_EXPORT int64_t bz_engine_workspace_bytes(const bz_engine_cfg* cfg) {
    if (!cfg_guard("bz_engine_workspace_bytes", cfg)) return -1;
    return carve(*cfg).total;
}

BZ_EXPORT int32_t bz_engine_create(const bz_engine_cfg* cfg, void* ws, int64_t bytes, bz_engine** out) {
    BZ_REQUIRE(ws && out, "bz_engine_create: null pointer");
    if (!cfg_guard("bz_engine_create", cfg)) return BZ_EINVAL;
    if (bz_device_count() <= 0) { set_error("bz_engine_create: no HIP device (the engine has no CPU path)"); return BZ_ENOGPU; }
    Offsets o = carve(*cfg);
    if (bytes < o.total) { set_error("bz_engine_create: workspace too small (%lld < %lld)", (long long)bytes, (long long)o.total); return BZ_ENOMEM; }
    BZ_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "bz_engine_create: workspace must be 256-byte aligned");
    bz_engine* e = new (std::nothrow) bz_engine();
    if (!e) { set_error("out of host memory"); return BZ_ENOMEM; }
    e->cfg = *cfg; e->net = nullptr; e->mlp = nullptr; e->bytes = o.total; e->pack_parity = 1; e->n_ahead = 0; e->search_seq = 0; e->eval_epoch = 0;
    e->sym_on = 0; e->sym_seed = 0;
    e->replay_seed = 2; e->paced = 0; e->seed_from_prev = 0; e->seed_src = 0;
    e->gumbel = GumbelDev{};  // off
    e->gin = GumbelInDev{};
    e->cap = CapDev{};
    e->forced = ForcedDev{};
    e->surp = SurpDev{};
    e->value = ValueDev{};
    e->own = OwnDev{};
    e->resign = ResignDev{}; e->resign_bytes = 0;
    e->store = StoreDev{}; e->store_index_bytes = 0;
    e->fpu = FpuDev{}; e->fpu_done = 0;
    e->solve = SolveDev{}; e->solve_bytes = 0;
    e->stop = StopDev{}; e->stop_host_exit = 0; e->stop_ring = nullptr;
    // measured on MI355X at 65,536 games x 50 sims: round 2 (profiles/r02_bench_ttt_gw*) 2 lanes 0.185 ms, 4 lanes 0.190 ms,
    // 8 lanes 0.294 ms per launch; round 3, after the kernel became issue-bound and lost a third of its instructions
    // (profiles/r03_bench_ttt_lanes.txt): 1 lane 0.162, 2 lanes 0.137, 4 lanes 0.134, 8 lanes 0.181 ms -> 4 lanes
    e->ttt_gw = cfg->ttt_lanes > 0 ? cfg->ttt_lanes : (cfg->ttt_lanes < 0 ? 0 : 4);
    EngineDev& d = e->dev;
    d.B = cfg->n_games; d.ncap = o.ncap; d.ecap = o.ecap; d.sims = cfg->sims; d.na = o.na; d.t_max = cfg->t_max;
    d.rounds = cfg->rounds; d.temp_moves = cfg->temp_moves; d.openings = cfg->openings; d.maxd = o.maxd;
    d.stagger = cfg->stagger;
    d.c_puct = cfg->c_puct; d.dir_alpha = cfg->dirichlet_alpha; d.dir_eps = cfg->dirichlet_eps; d.seed = cfg->seed; d.id_base = cfg->game_id_base; d.id_stride = cfg->game_id_stride;
    d.nodes = at<Node>(ws, o.nodes); d.edges = at<Edge>(ws, o.edges);
    d.reuse = (cfg->flags & BZ_ENGINE_REUSE_SUBTREE) ? 1 : 0;
    d.nodes_alt = at<Node>(ws, o.nodes_alt); d.edges_alt = at<Edge>(ws, o.edges_alt);
    d.g_reuse = at<u32>(ws, o.g_reuse);
    d.g_own = at<u64>(ws, o.g_own); d.g_opp = at<u64>(ws, o.g_opp); d.g_to_move = at<int8_t>(ws, o.g_to_move);
    d.g_state = at<uint8_t>(ws, o.g_state); d.g_moves = at<int32_t>(ws, o.g_moves); d.g_nex = at<int32_t>(ws, o.g_nex);
    d.g_round = at<int32_t>(ws, o.g_round); d.g_passes = at<int32_t>(ws, o.g_passes);
    d.hot = at<GameHot>(ws, o.hot); d.path = at<PathEnt>(ws, o.path);
    d.K = leaves_per_step(*cfg); d.lrec = at<LeafRec>(ws, o.lrec);
    d.leaf_kind = at<uint8_t>(ws, o.leaf_kind);
    d.leaf_own = at<u64>(ws, o.leaf_own); d.leaf_opp = at<u64>(ws, o.leaf_opp);
    d.c_own = at<u64>(ws, o.c_own); d.c_opp = at<u64>(ws, o.c_opp);
    d.compact = (net_eval(cfg->eval_kind) || mlp_eval(cfg->eval_kind)) ? 1 : 0;
    d.ecache = o.ecache; d.tt_buckets = o.tt_buckets; d.tt = at<u64>(ws, o.tt); d.node_v = at<float>(ws, o.node_v); d.node_v_alt = at<float>(ws, o.node_v_alt);
    if (o.ecache) {  // generation 0 = never written
        hipError_t ce = hipMemset(d.tt, 0, (size_t)cfg->n_games * o.tt_buckets * 16 * 8);
        if (ce != hipSuccess) { delete e; return hip_fail(ce, "bz_engine_create: evaluation-cache clear"); }
    }
    d.logits = at<float>(ws, o.logits); d.value = at<float>(ws, o.value);
    d.ex_own = at<u64>(ws, o.ex_own); d.ex_opp = at<u64>(ws, o.ex_opp); d.ex_pi = at<float>(ws, o.ex_pi);
    d.ex_z = at<int8_t>(ws, o.ex_z); d.ex_mover = at<int8_t>(ws, o.ex_mover); d.ex_act = at<uint8_t>(ws, o.ex_act);
    d.ex_len = at<int32_t>(ws, o.ex_len); d.ex_winner = at<int8_t>(ws, o.ex_winner);
    d.root_N = at<u32>(ws, o.root_N); d.root_W = at<float>(ws, o.root_W); d.root_P = at<float>(ws, o.root_P);
    d.counters = at<u64>(ws, o.counters); d.flags = at<u32>(ws, o.flags);
    d.cnt_slots = at<u64>(ws, o.cnt_slots); d.n_cnt_slots = o.n_cnt_slots;
    d.pack_off = at<int32_t>(ws, o.pack_off);
    bz_engine_layout& l = e->lay;
    l.ex_own = o.ex_own; l.ex_opp = o.ex_opp; l.ex_pi = o.ex_pi; l.ex_z = o.ex_z; l.ex_mover = o.ex_mover;
    l.ex_act = o.ex_act; l.ex_len = o.ex_len; l.ex_winner = o.ex_winner; l.root_N = o.root_N; l.root_W = o.root_W;
    l.root_P = o.root_P; l.leaf_own = o.leaf_own; l.leaf_opp = o.leaf_opp; l.leaf_kind = o.leaf_kind;
    l.logits = o.logits; l.value = o.value; l.g_own = o.g_own; l.g_opp = o.g_opp; l.g_to_move = o.g_to_move;
    l.g_state = o.g_state; l.counters = o.counters; l.na = o.na; l.t_max = cfg->t_max;
    l.ex_begin = o.ex_own; l.ex_bytes = o.ex_meta + 256 - o.ex_own; l.ex_meta = o.ex_meta;
    {   // self-describing header of the example block (so a gathered block can be unpacked without its engine)
        uint64_t meta[32] = {0};
        meta[0] = 0x425A455841000002ULL;  // "BZEXA" + layout version 2
        meta[1] = cfg->game_id_base; meta[2] = cfg->game_id_stride; meta[3] = (uint64_t)cfg->n_games;
        meta[4] = (uint64_t)cfg->rounds; meta[5] = (uint64_t)cfg->t_max; meta[6] = (uint64_t)o.na; meta[7] = (uint64_t)cfg->game;
        const int64_t offs[8] = {o.ex_own, o.ex_opp, o.ex_pi, o.ex_z, o.ex_mover, o.ex_act, o.ex_len, o.ex_winner};
        for (int i = 0; i < 8; ++i) meta[8 + i] = (uint64_t)(offs[i] - o.ex_own);
        hipError_t me = hipMemcpy(at<char>(ws, o.ex_meta), meta, sizeof(meta), hipMemcpyHostToDevice);
        if (me != hipSuccess) { delete e; return hip_fail(me, "bz_engine_create: example header upload"); }
    }
    *out = e;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_destroy(bz_engine* e) {
    if (e) for (int i = 0; i < e->n_ahead; ++i) (void)hipEventDestroy(e->ahead[i]);
    if (e && e->stop_ring) (void)hipHostFree(e->stop_ring);
    delete e;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_get_layout(const bz_engine* e, bz_engine_layout* out) {
    BZ_REQUIRE(e && out, "bz_engine_get_layout: null pointer");
    *out = e->lay;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_set_net(bz_engine* e, bz_net* net) {
    BZ_REQUIRE(e, "bz_engine_set_net: null engine");
    BZ_REQUIRE(e->dev.K == 1 || !net || (int64_t)bz_net_max_batch(net) >= (int64_t)e->dev.K * e->dev.B,
               "bz_engine_set_net: the net's max_batch is below leaves_per_step x n_games (the evaluator rows of one step)");
    e->net = net;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_set_mlp(bz_engine* e, bz_mlp* mlp) {
    BZ_REQUIRE(e, "bz_engine_set_mlp: null engine");
    BZ_REQUIRE(e->dev.K == 1 || !mlp || (int64_t)bz_mlp_max_batch(mlp) >= (int64_t)e->dev.K * e->dev.B,
               "bz_engine_set_mlp: the MLP's max_batch is below leaves_per_step x n_games (the evaluator rows of one step)");
    e->mlp = mlp;
    return BZ_OK;
}

/* Hashed evaluation symmetry: on != 0 -> bz_engine_evaluate runs the net's HASHED forward with `seed`; the
 * evaluator stays a function of the position, so the cache, the carry-over and every search option keep their guarantees.
 * A change of the setting or of the seed is a change of evaluator: like a change of weights, nothing is carried over it. */
BZ_EXPORT int32_t bz_engine_set_eval_symmetry(bz_engine* e, int32_t on, uint64_t seed) {
    BZ_REQUIRE(e, "bz_engine_set_eval_symmetry: null engine");
    on = on != 0;
    if (!on) seed = 0;
    BZ_REQUIRE(!on || (net_eval(e->cfg.eval_kind) && e->cfg.game != BZ_GAME_TTT),
               "bz_engine_set_eval_symmetry: the evaluation symmetry serves the net_f32 / net_bf16 / net_fp8 evaluators on the Reversi boards");
    if (on != e->sym_on || seed != e->sym_seed) e->eval_epoch = 0;  // no net has epoch 0
    e->sym_on = on; e->sym_seed = seed;
    return BZ_OK;
}

/* The replay seed: mode 1 -> a plain search with the carry-over starts every slot from the played child's old
 * subtree and paces its remaining walks over the move's launches; 0 -> every search is stepped as before; 2 (the default) -> 1 for
 * an engine of more than 1024 slots, where levelling the launches pays, else 0.  No result and no counter depends on the setting.
 * Takes effect with the next search. */
BZ_EXPORT int32_t bz_engine_set_replay_seed(bz_engine* e, int32_t mode) {
    BZ_REQUIRE(e && mode >= 0 && mode <= 2, "bz_engine_set_replay_seed: null engine, or mode not 0 (off), 1 (on) or 2 (by the engine's size)");
    e->replay_seed = mode;
    return BZ_OK;
}

/* the pacing rule of a replay-seeded slot (csrc/bz_pace.h, the code k_pace_step runs) over the launches 0 .. sims - 1 of a move, for
 * a slot with r <= sims walks left: walk[L] = 1 iff the slot walks in launch L, done[L] = the walks it made before launch L */
BZ_EXPORT int32_t bz_pace_walk(int32_t sims, int32_t r, uint8_t* walk, uint32_t* done) {
    BZ_REQUIRE(walk && done && sims >= 1 && sims <= BZ_ENGINE_MAX_SIMS && r >= 0 && r <= sims,
               "bz_pace_walk: null pointer, sims outside 1 .. 8189 or r outside 0 .. sims");
    for (int32_t L = 0; L < sims; ++L) {
        walk[L] = pace_walks((u32)L, (u32)r, (u32)sims) ? 1 : 0;
        done[L] = pace_done((u32)L, (u32)r, (u32)sims);
    }
    return BZ_OK;
}

/* test hook: the number of searches begun so far, as the evaluation cache counts them (its generation stamp cycles through
 * 1 .. 2^19 - 2).  Lets a test start an engine just below the wrap instead of running half a million searches. */
BZ_EXPORT int32_t bz_engine_debug_set_search_seq(bz_engine* e, uint32_t seq) {
    BZ_REQUIRE(e, "null engine");
    BZ_REQUIRE(seq < kTtGenMax - 1u, "bz_engine_debug_set_search_seq: 0 <= seq <= 2^19 - 3");
    e->search_seq = seq;
    e->eval_epoch = 0;  // nothing is carried over from before the jump
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_reset_counters(bz_engine* e, void* stream) {
    BZ_REQUIRE(e, "null engine");
    BZ_HIP(hipMemsetAsync(e->dev.counters, 0, kCntWords * 8, (hipStream_t)stream));
    BZ_HIP(hipMemsetAsync(e->dev.cnt_slots, 0, (size_t)e->dev.n_cnt_slots * CNT_N * 8, (hipStream_t)stream));
    return BZ_OK;
}

/* fold the per-wave counter slots into the counters[16] array of the layout (async) */
BZ_EXPORT int32_t bz_engine_sum_counters(bz_engine* e, void* stream) {
    BZ_REQUIRE(e, "null engine");
    hipLaunchKernelGGL(k_sum_counters, dim3(1), dim3(256), 0, (hipStream_t)stream, e->dev);
    BZ_LAUNCH_CHECK("k_sum_counters");
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_reset_games(bz_engine* e, void* stream) {
    BZ_REQUIRE(e, "null engine");
    BZ_DISPATCH(e, k_reset_games, stream, e->dev);
    if (e->own.fin_x)  //  no game is finished: every final board 0 (fin_x and fin_o are one range)
        BZ_HIP(hipMemsetAsync(e->own.fin_x, 0, (size_t)(reinterpret_cast<char*>(e->own.pi) - reinterpret_cast<char*>(e->own.fin_x)),
                              (hipStream_t)stream));
    if (e->resign.streak)  //  no streak, no record
        BZ_HIP(hipMemsetAsync(e->resign.streak, 0, (size_t)e->resign_bytes, (hipStream_t)stream));
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_set_roots(bz_engine* e, const uint64_t* own, const uint64_t* opp, const int8_t* to_move,
                                      void* stream) {
    BZ_REQUIRE(e && own && opp && to_move, "bz_engine_set_roots: null pointer");
    hipLaunchKernelGGL(k_set_roots, grid_of(e->dev.B), dim3(256), 0, (hipStream_t)stream, e->dev, own, opp, to_move);
    BZ_LAUNCH_CHECK("k_set_roots");
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_root_begin(bz_engine* e, void* stream) {
    BZ_REQUIRE(e, "null engine");
    // evaluations of the previous search are this search's only under the same weights (bz_net_update / bz_engine_set_net between
    // two searches of a live engine: nothing is carried over, exactly as if the slot had sat the previous search out)
    const uint64_t epoch = bz_net_epoch(e->net);
    const int carry_ok = epoch == e->eval_epoch;
    e->eval_epoch = epoch;
    if (e->store.S > 0) {  //  the root store lives and dies with the carry-over: another evaluator, an empty store
        if (!carry_ok) BZ_HIP(hipMemsetAsync(e->store.n_used, 0, (size_t)e->store_index_bytes, (hipStream_t)stream));
        else if (e->search_seq != 0u) {  // ... else the stored trees of the next roots, in the arena that is about to become the previous one
            hipLaunchKernelGGL(k_store_seed, dim3(e->dev.B), dim3(256), 0, (hipStream_t)stream, e->dev, e->store, e->search_seq, epoch);
            BZ_LAUNCH_CHECK("k_store_seed");
        }
    }
    e->search_seq = e->search_seq % (kTtGenMax - 1u) + 1u;  // 1 .. 2^19 - 2 (0 = never written)
    if (e->dev.ecache == 2) {  // the tree just searched stays intact in the other arena while the new one grows in this one
        Node* tn = e->dev.nodes; e->dev.nodes = e->dev.nodes_alt; e->dev.nodes_alt = tn;
        Edge* te = e->dev.edges; e->dev.edges = e->dev.edges_alt; e->dev.edges_alt = te;
        float* tv = e->dev.node_v; e->dev.node_v = e->dev.node_v_alt; e->dev.node_v_alt = tv;
    }
    BZ_DISPATCH(e, k_root_begin, stream, e->dev, e->search_seq, carry_ok);
    if (e->cap.fast > 0) {  // this search's budgets
        hipLaunchKernelGGL(k_cap_budget, grid_of(e->dev.B), dim3(256), 0, (hipStream_t)stream, e->dev, e->cap);
        BZ_LAUNCH_CHECK("k_cap_budget");
    }
    e->pack_parity = 1;
    e->fpu_done = 0;
    e->paced = 0;  // (paced_search, behind this call, says otherwise)
    e->seed_src = e->seed_from_prev; e->seed_from_prev = 0;
    if (e->solve.root)  //  no root is decided, both counts 0
        BZ_HIP(hipMemsetAsync(e->solve.root, 0, (size_t)e->solve_bytes, (hipStream_t)stream));
    if (e->stop.stop_at) {  //  every slot with a root: its whole budget; the others: 0; no step has walked
        hipLaunchKernelGGL(k_stop_begin, grid_of(e->dev.B), dim3(256), 0, (hipStream_t)stream, e->dev, e->stop);
        BZ_LAUNCH_CHECK("k_stop_begin");
    }
    return BZ_OK;
}

// The engine's search mode (Mode): the bits of the options that are on (option_on).  The setters refuse every combination Mode
// refuses, so what comes out is one of the masks tree_step() and bz_engine_play() switch over.
static unsigned engine_mode(const bz_engine* e) {
    unsigned m = 0u;
    for (int o = 0; o < BZ_OPT_COUNT; ++o) m |= option_on(e, o) ? kOptions[o].mode : 0u;
    return m;
}
// every slot's budget for the observers of a search: null without playout cap randomisation (every search is a full one)
static const u32* cap_budgets(const bz_engine* e) { return e->cap.fast > 0 ? static_cast<const u32*>(e->cap.budget) : nullptr; }

static int32_t tree_step(bz_engine* e, int do_expand, int do_select, uint32_t sim_idx, void* stream) {
    ProfScope ps(do_select ? BZ_PROF_SELECT : BZ_PROF_EXPAND_BACKUP, stream);
    const unsigned m = engine_mode(e) | (e->paced ? kModePace : 0u);  // (paced_search: only the plain mode is ever paced)
    //  the FPU kernels take sim_idx = simulations backed up after this step, on an expand-only step too
    if ((m & kModeFpu) && !do_select) sim_idx = (uint32_t)e->fpu_done;
#define BZ_STEP(KERNEL, ...) BZ_DISPATCH_G(e, KERNEL, stream, __VA_ARGS__, do_expand, do_select, sim_idx); break
    switch (m) {
    case 0u: BZ_STEP(k_tree_step, e->dev);
    case kModePace: BZ_STEP(k_pace_step, e->dev);  // 
    case kModeLeaf: BZ_STEP(k_leaf_step, e->dev);  // 
    case kModeGumbel: BZ_STEP(k_gumbel_step, e->dev, e->gumbel);  // 
    case kModeGumbel | kModeGfull: BZ_STEP(k_gfull_step, e->dev, e->gumbel, e->gin);  // 
    case kModeCap: BZ_STEP(k_cap_step, e->dev, e->cap);  // 
    case kModeForced: BZ_STEP(k_forced_step, e->dev, e->forced);  // 
    case kModeForced | kModeCap: BZ_STEP(k_forced_cap_step, e->dev, e->cap, e->forced);
    case kModeFpu: BZ_STEP(k_fpu_step, e->dev, e->fpu);  // 
    case kModeFpu | kModeCap: BZ_STEP(k_fpu_cap_step, e->dev, e->cap, e->fpu);
    case kModeFpu | kModeForced: BZ_STEP(k_fpu_forced_step, e->dev, e->forced, e->fpu);
    case kModeFpu | kModeForced | kModeCap: BZ_STEP(k_fpu_forced_cap_step, e->dev, e->cap, e->forced, e->fpu);
    case kModeSolve: BZ_STEP(k_solve_step, e->dev, e->solve);  // 
    case kModeSolve | kModeCap: BZ_STEP(k_solve_cap_step, e->dev, e->cap, e->solve);
    case kModeStop: BZ_STEP(k_stop_step, e->dev, e->stop);  // 
    case kModeFpu | kModeStop: BZ_STEP(k_fpu_stop_step, e->dev, e->fpu, e->stop);
    default: set_error("tree_step: no step kernel serves search mode 0x%x", m); return BZ_EINVAL;
    }
#undef BZ_STEP
    if (do_select) {  // leaf-parallel: sim_idx is a multiple of K, the packed-leaf buffers alternate per step
        e->pack_parity = (int)(((m & kModeLeaf) ? sim_idx / (uint32_t)e->dev.K : sim_idx) & 1u);
        if (m & kModeFpu) e->fpu_done = (int)sim_idx + 1;
    }
    return BZ_OK;
}

/* sim_index = number of simulations already completed in this search (the root's visit sum); with K leaves per step
 * 0, K, 2K, ...: the step starts the next min(K, sims - sim_index) walks */
BZ_EXPORT int32_t bz_engine_select(bz_engine* e, uint32_t sim_index, void* stream) {
    BZ_REQUIRE(e, "null engine");
    BZ_REQUIRE(e->dev.K == 1 || (sim_index % (uint32_t)e->dev.K == 0 && sim_index < (uint32_t)e->cfg.sims),
               "bz_engine_select: sim_index must be a multiple of leaves_per_step below sims");
    return tree_step(e, 0, 1, sim_index, stream);
}

BZ_EXPORT int32_t bz_engine_evaluate(bz_engine* e, void* stream) {
    BZ_REQUIRE(e, "null engine");
    int ek = e->cfg.eval_kind;
    if (ek == BZ_EVAL_UNIFORM || ek == BZ_EVAL_HASH) {
        BZ_DISPATCH(e, k_eval_synth, stream, e->dev, ek);
        return BZ_OK;
    }
    if (ek == BZ_EVAL_EXTERNAL) return BZ_OK;
    if (mlp_eval(ek)) {  // (cfg_ok: tic-tac-toe only) the packed leaves; value 0 from the reference's net, which has no value head, the net's own from a PV handle
        BZ_REQUIRE(e->mlp, "bz_engine_evaluate: eval_kind needs an MLP (bz_engine_set_mlp)");
        return bz_mlp_forward_dev(e->mlp, ek == BZ_EVAL_MLP_BF16 ? 1 : 0, e->dev.c_own, e->dev.c_opp, nullptr, e->dev.B * e->dev.K,
                                  e->dev.flags + FLAG_NEVAL + e->pack_parity, e->dev.logits, e->dev.value, stream);
    }
    BZ_REQUIRE(e->net, "bz_engine_evaluate: eval_kind needs a net (bz_engine_set_net)");
    // the net works on 8x8 planes; the reference's 6x6 / 4x4 boards live in their top-left corner (bit = 8*row+col for
    // every size), cells outside are never stones and never legal, so the same net serves them
    BZ_REQUIRE(e->cfg.game != BZ_GAME_TTT, "bz_engine_evaluate: the conv net serves the Reversi boards, not tic-tac-toe");
    // leaves were packed by select: evaluate only the first flags[NEVAL] slots (device-side count)
    const int kind = ek == BZ_EVAL_NET_BF16 ? 1 : (ek == BZ_EVAL_NET_FP8 ? 2 : 0);
    if (e->sym_on)  // every leaf under the symmetry its position and the seed hash to
        return bz_net_forward_sym_dev(e->net, kind, e->dev.c_own, e->dev.c_opp, e->dev.B * e->dev.K, e->dev.flags + FLAG_NEVAL + e->pack_parity,
                                      e->cfg.game == BZ_GAME_REVERSI6 ? 6 : (e->cfg.game == BZ_GAME_REVERSI4 ? 4 : 8), BZ_SYM_HASHED,
                                      e->sym_seed, nullptr, 0, e->dev.logits, e->dev.value, stream);
    return bz_net_forward_dev(e->net, ek == BZ_EVAL_NET_BF16 ? 1 : (ek == BZ_EVAL_NET_FP8 ? 2 : 0), e->dev.c_own, e->dev.c_opp, e->dev.B * e->dev.K,
                              e->dev.flags + FLAG_NEVAL + e->pack_parity, e->dev.logits, e->dev.value, stream);
}

BZ_EXPORT int32_t bz_engine_expand_backup(bz_engine* e, void* stream) {
    BZ_REQUIRE(e, "null engine");
    return tree_step(e, 1, 0, 0, stream);
}

/* Dirichlet noise on the priors of every active slot's (expanded) root -- a no-op when cfg.dirichlet_eps == 0 -- and, with
 * Gumbel root search on (bz_engine_set_gumbel), the search's Gumbel preparation of the expanded roots (k_gumbel_root).
 * Step-API order: root_begin, evaluate, expand_backup, root_noise, then select(0) ... -- what bz_engine_search does. */
BZ_EXPORT int32_t bz_engine_root_noise(bz_engine* e, void* stream) {
    BZ_REQUIRE(e, "null engine");
    //  the raw priors, before the noise rewrites them; without noise nothing ever does and bz_engine_play saves them
    if (e->surp.prior && e->dev.dir_eps > 0.0f) BZ_DISPATCH(e, k_surp_save, stream, e->dev, e->surp);
    if (e->gumbel.m > 0) BZ_DISPATCH(e, k_gumbel_root, stream, e->dev, e->gumbel);
    if (!(e->dev.dir_eps > 0.0f)) return BZ_OK;
    if (e->cap.fast > 0) {  // playout cap randomisation: the full searches only
        hipLaunchKernelGGL(k_cap_noise, dim3((e->dev.B + 63) / 64), dim3(64), 0, (hipStream_t)stream, e->dev, e->cap);
        BZ_LAUNCH_CHECK("k_cap_noise");
        return BZ_OK;
    }
    hipLaunchKernelGGL(k_root_noise, dim3((e->dev.B + 63) / 64), dim3(64), 0, (hipStream_t)stream, e->dev);
    BZ_LAUNCH_CHECK("k_root_noise");
    return BZ_OK;
}

// the roots are expanded on their own and bz_engine_root_noise runs before the first walk: Dirichlet noise, Gumbel root search
static bool root_prep(const bz_engine* e) { return e->dev.dir_eps > 0.0f || e->gumbel.m > 0; }
// an engine whose whole search is one launch (k_search_fused / k_search_fused_ttt; bz_engines_step: nothing to interleave): a
// synthetic evaluator, no subtree reuse, no root preparation and the plain search mode -- every mode's rule lives in the step
// kernels only
static bool search_is_fused(const bz_engine* e) {
    const int ek = e->cfg.eval_kind;
    return (ek == BZ_EVAL_UNIFORM || ek == BZ_EVAL_HASH) && !e->dev.reuse && !root_prep(e) && engine_mode(e) == 0u;
}

// ("The replay seed") behind bz_engine_root_begin of a search this file drives from its first step to its last:
// where the carry-over is on and the search is otherwise plain, the search is paced -- k_replay_seed gives every slot its seeded
// count (0 where nothing can be seeded: always, when the previous search was not such a search itself) and the steps are
// k_pace_step's.  Everything else runs as it always did.
// Levelling pays where a launch's time follows its rows.  The tower's throughput shape holds 4 positions per workgroup on 256 CUs:
// a pipeline of up to 1024 slots finishes ANY of its launches in one round of workgroups, a levelled launch costs it what a dense
// one does, and all the pacing does is trade the ~100 cheap latency-shape launches at the head of a move for full-price ones
// (measured: 2 x 1024 slots -2.2 %, 2 x 512 slots -8.6 % games per second, 2 x 2048 +1.8 %).
constexpr int kPaceAutoSlots = 1024;
static int32_t paced_search(bz_engine* e, void* stream) {
    const int from_prev = e->seed_src;
    const bool plain = engine_mode(e) == 0u && !(e->dev.dir_eps > 0.0f) && !e->dev.reuse && !e->sym_on && e->dev.ecache == 2 &&
                       net_eval(e->cfg.eval_kind) && e->cfg.game != BZ_GAME_TTT && e->dev.compact;
    if (!plain || e->replay_seed == 0 || (e->replay_seed == 2 && e->dev.B <= kPaceAutoSlots)) return BZ_OK;
    const size_t lds = (size_t)e->dev.ncap * 8;  // (ncap <= 8191: below the 64 KiB a block gets without asking)
    const u32* mark = e->store.S > 0 ? e->store.mark : nullptr;
#define BZ_SEED(G) hipLaunchKernelGGL(k_replay_seed<G>, dim3(e->dev.B), dim3(G::GW), lds, (hipStream_t)stream, e->dev, e->search_seq, from_prev, mark)
    switch (e->cfg.game) {
    case BZ_GAME_REVERSI6: BZ_SEED(Reversi6); break;
    case BZ_GAME_REVERSI4: BZ_SEED(Reversi4); break;
    default: BZ_SEED(Reversi); break;
    }
#undef BZ_SEED
    BZ_LAUNCH_CHECK("k_replay_seed");
    e->paced = 1;
    return BZ_OK;
}

//  behind the last tree step of a stepwise search: the finished trees of early roots go to the root store
static int32_t store_save(bz_engine* e, void* stream) {
    if (e->store.S == 0) return BZ_OK;
    hipLaunchKernelGGL(k_store_save, dim3(e->dev.B + 1), dim3(256), 0, (hipStream_t)stream, e->dev, e->store, e->search_seq, e->eval_epoch,
                       cap_budgets(e));
    BZ_LAUNCH_CHECK("k_store_save");
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_search(bz_engine* e, void* stream) {
    BZ_REQUIRE(e, "null engine");
    int ek = e->cfg.eval_kind;
    // (Dirichlet noise and Gumbel root search: the roots are expanded on their own and prepared before the first walk)
    const bool noise = root_prep(e);
    if (search_is_fused(e)) {
        ProfScope ps(BZ_PROF_SEARCH_FUSED, stream);
        if (e->cfg.game == BZ_GAME_TTT && e->cfg.sims <= kTttFusedMaxSims && e->ttt_gw > 0) {
            const dim3 grid = grid_groups(e->dev.B, e->ttt_gw);
#define BZ_TTT_FUSED(GWN)                                                                                              \
    do {                                                                                                                \
        if (ek == BZ_EVAL_UNIFORM) hipLaunchKernelGGL((k_search_fused_ttt<GWN, true>), grid, dim3(256), 0, (hipStream_t)stream, e->dev); \
        else hipLaunchKernelGGL((k_search_fused_ttt<GWN, false>), grid, dim3(256), 0, (hipStream_t)stream, e->dev);     \
    } while (0)
            switch (e->ttt_gw) {
            case 1: BZ_TTT_FUSED(1); break;
            case 2: BZ_TTT_FUSED(2); break;
            case 8: BZ_TTT_FUSED(8); break;
            default: BZ_TTT_FUSED(4); break;
            }
#undef BZ_TTT_FUSED
            BZ_LAUNCH_CHECK("k_search_fused_ttt");
            return BZ_OK;
        }
        BZ_DISPATCH_G(e, k_search_fused, stream, e->dev, ek);
        return BZ_OK;
    }
    BZ_REQUIRE(ek != BZ_EVAL_EXTERNAL, "bz_engine_search: BZ_EVAL_EXTERNAL callers drive the step API");
    int32_t rc;
    if ((rc = bz_engine_root_begin(e, stream)) != BZ_OK) return rc;
    if ((rc = paced_search(e, stream)) != BZ_OK) return rc;
    if ((rc = bz_engine_evaluate(e, stream)) != BZ_OK) return rc;
    if (noise) {  // expand the roots on their own, then draw the noise, then start selecting
        if ((rc = tree_step(e, 1, 0, 0, stream)) != BZ_OK) return rc;
        if ((rc = bz_engine_root_noise(e, stream)) != BZ_OK) return rc;
    }
    // expand+backup of the previous step's leaves (s = 0: the root) fused with the select of walks s .. s + K - 1
    for (int s = 0; s < e->cfg.sims; s += e->dev.K) {
        if ((rc = tree_step(e, (noise && s == 0) ? 0 : 1, 1, (uint32_t)s, stream)) != BZ_OK) return rc;
        if ((rc = bz_engine_evaluate(e, stream)) != BZ_OK) return rc;
    }
    if ((rc = tree_step(e, 1, 0, 0, stream)) != BZ_OK) return rc;
    e->seed_from_prev = e->paced;
    return store_save(e, stream);
}

BZ_EXPORT int32_t bz_engine_root_stats(bz_engine* e, void* stream) {
    BZ_REQUIRE(e, "null engine");
    BZ_DISPATCH(e, k_root_stats, stream, e->dev);
    return BZ_OK;
}

/* ---- Gumbel root search */
BZ_EXPORT int32_t bz_gumbel_considered_visits(int32_t n_considered, int32_t sims, uint16_t* out) {
    BZ_REQUIRE(out, "bz_gumbel_considered_visits: null pointer");
    BZ_REQUIRE(n_considered >= 1 && n_considered <= BZ_GUMBEL_MAX_CONSIDERED && sims >= 1 && sims <= BZ_ENGINE_MAX_SIMS,
               "bz_gumbel_considered_visits: n_considered must be in 1..64 and sims in 1..8189");
    if (n_considered <= 1) {
        for (int k = 0; k < sims; ++k) out[k] = (uint16_t)k;
        return BZ_OK;
    }
    // mctx's get_sequence_of_considered_visits: rounds of sequential halving, each giving every considered action
    // max(1, sims / (log2max * considered)) more visits, the considered count halving down to 2
    int log2max = 0;
    while ((1 << log2max) < n_considered) ++log2max;  // ceil(log2(n_considered))
    int visits[BZ_GUMBEL_MAX_CONSIDERED] = {0};
    int len = 0, nc = n_considered;
    while (len < sims) {
        const int q = sims / (log2max * nc), extra = q > 1 ? q : 1;
        for (int r = 0; r < extra; ++r) {
            for (int i = 0; i < nc; ++i) {
                if (len < sims) out[len] = (uint16_t)visits[i];
                ++len;
            }
            for (int i = 0; i < nc; ++i) visits[i]++;
        }
        nc = nc / 2 > 2 ? nc / 2 : 2;
    }
    return BZ_OK;
}

namespace {
struct GumbelOffsets { int64_t T, base, vroot, total; };
GumbelOffsets gumbel_carve(const bz_engine_cfg& c, int m) {
    GumbelOffsets o{};
    Carver k;
    const int64_t B = c.n_games, maxch = c.game == BZ_GAME_TTT ? TicTacToe::MAXCH : Reversi::MAXCH;
    o.T = k.take((int64_t)m * c.sims * 2);
    o.base = k.take(B * maxch * 4);
    o.vroot = k.take(B * 4);
    o.total = k.off;
    return o;
}
}  // namespace

BZ_EXPORT int64_t bz_engine_gumbel_bytes(const bz_engine_cfg* cfg, int32_t max_considered) {
    if (!cfg_guard("bz_engine_gumbel_bytes", cfg)) return -1;
    if (max_considered < 1 || max_considered > BZ_GUMBEL_MAX_CONSIDERED) {
        set_error("bz_engine_gumbel_bytes: max_considered must be in 1..64 (got %d)", (int)max_considered);
        return -1;
    }
    if (option_refusal("bz_engine_gumbel_bytes", BZ_OPT_GUMBEL, *cfg)) return -1;
    return gumbel_carve(*cfg, max_considered).total;
}

BZ_EXPORT int32_t bz_engine_set_gumbel(bz_engine* e, int32_t max_considered, float gumbel_scale, float maxvisit_init,
                                       float value_scale, void* buf, int64_t buf_bytes, void* stream) {
    BZ_REQUIRE(e, "bz_engine_set_gumbel: null engine");
    if (max_considered == 0) {  // off: the next search is a PUCT search again (and the interior rule goes with it)
        e->gumbel.m = 0;
        e->gin = GumbelInDev{};
        return BZ_OK;
    }
    BZ_REQUIRE(max_considered >= 1 && max_considered <= BZ_GUMBEL_MAX_CONSIDERED, "bz_engine_set_gumbel: max_considered must be in 0..64");
    const bool finite = __builtin_isfinite(gumbel_scale) && __builtin_isfinite(maxvisit_init) && __builtin_isfinite(value_scale);
    BZ_REQUIRE(finite && gumbel_scale >= 0.0f && maxvisit_init >= 0.0f && value_scale >= 0.0f,
               "bz_engine_set_gumbel: gumbel_scale, maxvisit_init and value_scale must be finite and >= 0");
    if (option_refusal("bz_engine_set_gumbel", BZ_OPT_GUMBEL, e)) return BZ_EINVAL;
    const GumbelOffsets o = gumbel_carve(e->cfg, max_considered);
    if (int32_t rc = option_buffer("bz_engine_set_gumbel", buf, buf_bytes, o.total)) return rc;
    // T [m][sims]: setup, not the hot path -- built on the host and uploaded once
    const int sims = e->cfg.sims;
    uint16_t* T = new (std::nothrow) uint16_t[(size_t)max_considered * sims];
    if (!T) { set_error("out of host memory"); return BZ_ENOMEM; }
    for (int nc = 1; nc <= max_considered; ++nc) (void)bz_gumbel_considered_visits(nc, sims, T + (size_t)(nc - 1) * sims);
    hipError_t he = hipMemcpyAsync(at<char>(buf, o.T), T, (size_t)max_considered * sims * 2, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (he == hipSuccess) he = hipStreamSynchronize((hipStream_t)stream);
    delete[] T;
    if (he != hipSuccess) return hip_fail(he, "bz_engine_set_gumbel: upload of the considered-visit table");
    GumbelDev& gd = e->gumbel;
    gd.m = max_considered; gd.scale = gumbel_scale; gd.mvi = maxvisit_init; gd.vs = value_scale;
    gd.T = at<uint16_t>(buf, o.T); gd.base = at<float>(buf, o.base); gd.vroot = at<float>(buf, o.vroot);
    return BZ_OK;
}

/* ---- Gumbel interior selection */
namespace {
inline int64_t gumbel_interior_bytes(const bz_engine_cfg& c) { Carver k; k.take((int64_t)c.n_games * nodes_per_game(c) * 4); return k.off; }
}  // namespace

BZ_EXPORT int64_t bz_engine_gumbel_interior_bytes(const bz_engine_cfg* cfg) {
    if (!cfg_guard("bz_engine_gumbel_interior_bytes", cfg)) return -1;
    if (option_refusal("bz_engine_gumbel_interior_bytes", BZ_OPT_GUMBEL, *cfg)) return -1;
    return gumbel_interior_bytes(*cfg);
}

BZ_EXPORT int32_t bz_engine_set_gumbel_interior(bz_engine* e, int32_t on, void* buf, int64_t buf_bytes, void* stream) {
    (void)stream;  // (nothing is uploaded or cleared: every node's value is written with its expansion before it is read)
    BZ_REQUIRE(e, "bz_engine_set_gumbel_interior: null engine");
    if (!on) {  // off: k_gumbel_step (or the PUCT kernels) again
        e->gin = GumbelInDev{};
        return BZ_OK;
    }
    BZ_REQUIRE(e->gumbel.m > 0, "bz_engine_set_gumbel_interior: the Gumbel interior rule needs Gumbel root search (bz_engine_set_gumbel first)");
    if (int32_t rc = option_buffer("bz_engine_set_gumbel_interior", buf, buf_bytes, gumbel_interior_bytes(e->cfg), BZ_EINVAL)) return rc;
    e->gin.node_v = static_cast<float*>(buf);
    return BZ_OK;
}

BZ_EXPORT int32_t bz_gumbel_interior_pick(const uint32_t* N, const float* W, const float* P, int32_t n, float v_node, float maxvisit_init,
                                          float value_scale, float* p_out, float* score_out) {
    if (!(N && W && P && n >= 1 && n <= kGiMaxN)) { set_error("bz_gumbel_interior_pick: null pointer or n outside 1 .. 64"); return -1; }
    if (n == 1) {  // a forced pass: the walk takes edge 0; the policy of one action
        if (p_out) p_out[0] = 1.0f;
        if (score_out) score_out[0] = gi_score(1.0f, N[0], 1.0f + (float)N[0]);
        return 0;
    }
    return gi_pick_serial(N, W, P, n, v_node, maxvisit_init, value_scale, p_out, score_out);
}

/* ---- playout cap randomisation */
namespace {
inline int64_t cap_bytes(const bz_engine_cfg& c) { Carver k; k.take((int64_t)c.n_games * 4); return k.off; }
}  // namespace

BZ_EXPORT int64_t bz_engine_playout_cap_bytes(const bz_engine_cfg* cfg) {
    if (!cfg_guard("bz_engine_playout_cap_bytes", cfg)) return -1;
    if (option_refusal("bz_engine_playout_cap_bytes", BZ_OPT_PLAYOUT_CAP, *cfg)) return -1;
    return cap_bytes(*cfg);
}

BZ_EXPORT int32_t bz_engine_set_playout_cap(bz_engine* e, int32_t fast_sims, uint32_t full_q, void* buf, int64_t bytes, void* stream) {
    BZ_REQUIRE(e, "bz_engine_set_playout_cap: null engine");
    if (fast_sims == 0) {  // off: every search has cfg.sims simulations and records its row again
        e->cap = CapDev{};
        return BZ_OK;
    }
    BZ_REQUIRE(fast_sims >= 1 && fast_sims < e->cfg.sims, "bz_engine_set_playout_cap: fast_sims must be 0 (off) or in 1 .. sims - 1");
    BZ_REQUIRE(full_q <= 65536u, "bz_engine_set_playout_cap: full_q must be in 0 .. 65536 (the probability of a full search in units of 2^-16)");
    if (option_refusal("bz_engine_set_playout_cap", BZ_OPT_PLAYOUT_CAP, e)) return BZ_EINVAL;
    if (int32_t rc = option_buffer("bz_engine_set_playout_cap", buf, bytes, cap_bytes(e->cfg))) return rc;
    BZ_HIP(hipMemsetAsync(buf, 0, (size_t)e->cfg.n_games * 4, (hipStream_t)stream));  // no search yet: no budgets
    e->cap.fast = fast_sims; e->cap.full_q = full_q; e->cap.budget = static_cast<u32*>(buf);
    return BZ_OK;
}

BZ_EXPORT int32_t bz_playout_cap_budget(uint64_t seed, uint64_t gid, uint32_t moves_made, int32_t sims, int32_t fast_sims, uint32_t full_q) {
    if (!(sims >= 2 && sims <= BZ_ENGINE_MAX_SIMS && fast_sims >= 1 && fast_sims < sims && full_q <= 65536u)) {
        set_error("bz_playout_cap_budget: need 1 <= fast_sims < sims <= %d and full_q in 0 .. 65536", (int)BZ_ENGINE_MAX_SIMS);
        return -1;
    }
    return (int32_t)cap_budget(seed, gid, (u64)moves_made, sims, fast_sims, full_q);
}

/* ---- forced playouts and policy target pruning */
namespace {
// the k forced playouts refuse (nullptr: none)
const char* forced_refusal(float k) { return k >= 0.0f && k <= 3.0e38f ? nullptr : "forced playouts: k must be finite and >= 0 (0 = off)"; }
}  // namespace

BZ_EXPORT int32_t bz_engine_forced_playouts_check(const bz_engine_cfg* cfg, float k) {
    if (!cfg_guard("bz_engine_forced_playouts_check", cfg)) return BZ_EINVAL;
    if (const char* why = forced_refusal(k)) { set_error("bz_engine_forced_playouts_check: %s", why); return BZ_EINVAL; }
    if (option_refusal("bz_engine_forced_playouts_check", BZ_OPT_FORCED_PLAYOUTS, *cfg)) return BZ_EINVAL;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_set_forced_playouts(bz_engine* e, float k, int32_t prune, void* stream) {
    (void)stream;  // (nothing is uploaded: k and the prune flag travel as kernel arguments)
    BZ_REQUIRE(e, "bz_engine_set_forced_playouts: null engine");
    if (k == 0.0f) {  // off: the plain (or the cap's) kernels again
        e->forced = ForcedDev{};
        return BZ_OK;
    }
    if (const char* why = forced_refusal(k)) { set_error("bz_engine_set_forced_playouts: %s", why); return BZ_EINVAL; }
    if (option_refusal("bz_engine_set_forced_playouts", BZ_OPT_FORCED_PLAYOUTS, e)) return BZ_EINVAL;
    e->forced.k = k; e->forced.prune = prune ? 1 : 0;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_forced_prune(const uint32_t* N, const float* W, const float* P, int32_t n, float c_puct, float k, uint32_t* N_out) {
    BZ_REQUIRE(N && W && P && N_out && n >= 1 && n <= 255, "bz_forced_prune: null pointer or n outside 1 .. 255");
    BZ_REQUIRE(k > 0.0f && k <= 3.0e38f, "bz_forced_prune: k must be finite and > 0");
    Edge ed[255];
    for (int i = 0; i < n; ++i) {
        if (N[i] > kNMask) { set_error("bz_forced_prune: N[%d] = %u exceeds %u", i, N[i], kNMask); return BZ_EINVAL; }
        ed[i].w0 = N[i]; ed[i].W = W[i]; ed[i].P = P[i]; ed[i].w3 = 0;
    }
    forced_prune(ed, n, c_puct, k, [N_out](int i, const Edge&, u32 Np) { N_out[i] = Np; });
    return BZ_OK;
}

/* ---- first-play urgency reduction */
namespace {
inline bool fpu_red_ok(float r) { return r >= 0.0f && r <= 3.0e38f; }  // (a NaN fails)
inline int64_t fpu_bytes(const bz_engine_cfg& c) { Carver k; k.take((int64_t)c.n_games * 4); return k.off; }
}  // namespace

BZ_EXPORT int64_t bz_engine_fpu_bytes(const bz_engine_cfg* cfg) {
    if (!cfg_guard("bz_engine_fpu_bytes", cfg)) return -1;
    if (option_refusal("bz_engine_fpu_bytes", BZ_OPT_FPU, *cfg)) return -1;
    return fpu_bytes(*cfg);
}

BZ_EXPORT int32_t bz_engine_fpu_check(const bz_engine_cfg* cfg, float reduction, float root_reduction) {
    if (!cfg_guard("bz_engine_fpu_check", cfg)) return BZ_EINVAL;
    BZ_REQUIRE(fpu_red_ok(reduction) && fpu_red_ok(root_reduction),
               "bz_engine_fpu_check: first-play urgency reduction: reduction and root_reduction must be finite and >= 0");
    if (option_refusal("bz_engine_fpu_check", BZ_OPT_FPU, *cfg)) return BZ_EINVAL;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_set_fpu(bz_engine* e, int32_t on, float reduction, float root_reduction, void* buf, int64_t bytes, void* stream) {
    BZ_REQUIRE(e, "bz_engine_set_fpu: null engine");
    if (!on) {  // off: the plain (the cap's, the forced) kernels again
        e->fpu = FpuDev{};
        return BZ_OK;
    }
    BZ_REQUIRE(fpu_red_ok(reduction) && fpu_red_ok(root_reduction),
               "bz_engine_set_fpu: first-play urgency reduction: reduction and root_reduction must be finite and >= 0");
    if (option_refusal("bz_engine_set_fpu", BZ_OPT_FPU, e)) return BZ_EINVAL;
    if (int32_t rc = option_buffer("bz_engine_set_fpu", buf, bytes, fpu_bytes(e->cfg))) return rc;
    BZ_HIP(hipMemsetAsync(buf, 0, (size_t)e->cfg.n_games * 4, (hipStream_t)stream));
    e->fpu.reduction = reduction; e->fpu.root_reduction = root_reduction; e->fpu.root_w = static_cast<float*>(buf);
    return BZ_OK;
}

BZ_EXPORT uint32_t bz_fpu_mass(const uint32_t* N, const float* P, int32_t n) {
    if (!(N && P && n >= 1 && n <= 255)) { set_error("bz_fpu_mass: null pointer or n outside 1 .. 255"); return 0xFFFFFFFFu; }
    for (int i = 0; i < n; ++i)  // (a prior is at most 1; 255 of them stay far below 2^32)
        if (P[i] > 2.0f) { set_error("bz_fpu_mass: P[%d] = %g is no prior (> 2)", i, (double)P[i]); return 0xFFFFFFFFu; }
    return fpu_mass(n, [N](int i) { return N[i]; }, [P](int i) { return P[i]; });
}

BZ_EXPORT float bz_fpu_value(const uint32_t* N, const float* P, int32_t n, float q_node, float reduction) {
    const uint32_t S = bz_fpu_mass(N, P, n);
    if (S == 0xFFFFFFFFu) return __builtin_nanf("");
    return fpu_value(S, q_node, reduction);
}

/* ---- proven wins, losses and draws */
namespace {
struct SolveOffsets { int64_t root, counts, total; };
inline SolveOffsets solver_carve(const bz_engine_cfg& c) {
    Carver k; SolveOffsets o;
    o.root = k.take((int64_t)c.n_games * 4); o.counts = k.take(8); o.total = k.off;
    return o;
}
}  // namespace

BZ_EXPORT int64_t bz_engine_solver_bytes(const bz_engine_cfg* cfg) {
    if (!cfg_guard("bz_engine_solver_bytes", cfg)) return -1;
    if (option_refusal("bz_engine_solver_bytes", BZ_OPT_SOLVER, *cfg)) return -1;
    return solver_carve(*cfg).total;
}

BZ_EXPORT int32_t bz_engine_solver_check(const bz_engine_cfg* cfg) {
    if (!cfg_guard("bz_engine_solver_check", cfg)) return BZ_EINVAL;
    if (option_refusal("bz_engine_solver_check", BZ_OPT_SOLVER, *cfg)) return BZ_EINVAL;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_set_solver(bz_engine* e, int32_t on, void* buf, int64_t bytes, void* stream) {
    BZ_REQUIRE(e, "bz_engine_set_solver: null engine");
    if (!on) {  // off: the plain (the cap's) kernels again
        e->solve = SolveDev{}; e->solve_bytes = 0;
        return BZ_OK;
    }
    if (option_refusal("bz_engine_set_solver", BZ_OPT_SOLVER, e)) return BZ_EINVAL;
    const SolveOffsets o = solver_carve(e->cfg);
    if (int32_t rc = option_buffer("bz_engine_set_solver", buf, bytes, o.total)) return rc;
    BZ_HIP(hipMemsetAsync(buf, 0, (size_t)o.total, (hipStream_t)stream));
    char* b = static_cast<char*>(buf);
    e->solve.root = reinterpret_cast<int32_t*>(b + o.root); e->solve.counts = reinterpret_cast<u32*>(b + o.counts);
    e->solve_bytes = o.total;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_root_proven(bz_engine* e, int8_t* edge_out, int8_t* root_out, uint32_t* counts_out, void* stream) {
    BZ_REQUIRE(e && edge_out && root_out && counts_out, "bz_engine_root_proven: null pointer");
    BZ_REQUIRE(e->solve.root, "bz_engine_root_proven: the solver is off (bz_engine_set_solver)");
    BZ_DISPATCH(e, k_solve_read, stream, e->dev, e->solve, edge_out, root_out);
    BZ_HIP(hipMemcpyAsync(counts_out, e->solve.counts, 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BZ_OK;
}

BZ_EXPORT int32_t bz_solver_node(const int8_t* vals, int32_t n) {
    if (!(vals && n >= 1 && n <= 255)) { set_error("bz_solver_node: null pointer or n outside 1 .. 255"); return -128; }
    for (int i = 0; i < n; ++i)
        if (vals[i] < -1 || vals[i] > 2) { set_error("bz_solver_node: vals[%d] = %d is none of -1, 0, +1, 2 (undecided)", i, (int)vals[i]); return -128; }
    return solver_node(n, [vals](int i) { return (int)vals[i]; });
}

BZ_EXPORT int32_t bz_solver_pick(const uint32_t* N, const int8_t* vals, int32_t n, int32_t tau1, uint64_t draw) {
    if (!(N && vals && n >= 1 && n <= 255)) { set_error("bz_solver_pick: null pointer or n outside 1 .. 255"); return -1; }
    for (int i = 0; i < n; ++i)
        if (vals[i] < -1 || vals[i] > 2) { set_error("bz_solver_pick: vals[%d] = %d is none of -1, 0, +1, 2 (undecided)", i, (int)vals[i]); return -1; }
    return solver_pick(n, [N](int i) { return (u64)N[i]; }, [vals](int i) { return (int)vals[i]; }, tau1 != 0, (u64)draw);
}

/* ---- exact early stop */
namespace {
struct StopOffsets { int64_t stop_at, walked, total; };
inline StopOffsets early_stop_carve(const bz_engine_cfg& c) {
    Carver k; StopOffsets o;
    o.stop_at = k.take((int64_t)c.n_games * 4); o.walked = k.take(4); o.total = k.off;
    return o;
}
}  // namespace

BZ_EXPORT int64_t bz_engine_early_stop_bytes(const bz_engine_cfg* cfg) {
    if (!cfg_guard("bz_engine_early_stop_bytes", cfg)) return -1;
    if (option_refusal("bz_engine_early_stop_bytes", BZ_OPT_EARLY_STOP, *cfg)) return -1;
    return early_stop_carve(*cfg).total;
}

BZ_EXPORT int32_t bz_engine_early_stop_check(const bz_engine_cfg* cfg) {
    if (!cfg_guard("bz_engine_early_stop_check", cfg)) return BZ_EINVAL;
    if (option_refusal("bz_engine_early_stop_check", BZ_OPT_EARLY_STOP, *cfg)) return BZ_EINVAL;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_set_early_stop(bz_engine* e, int32_t on, int32_t host_exit, void* buf, int64_t bytes, void* stream) {
    BZ_REQUIRE(e, "bz_engine_set_early_stop: null engine");
    if (!on) {  // off: the plain (the FPU) kernels again
        e->stop = StopDev{}; e->stop_host_exit = 0;
        return BZ_OK;
    }
    if (option_refusal("bz_engine_set_early_stop", BZ_OPT_EARLY_STOP, e)) return BZ_EINVAL;
    const StopOffsets o = early_stop_carve(e->cfg);
    if (int32_t rc = option_buffer("bz_engine_set_early_stop", buf, bytes, o.total)) return rc;
    BZ_HIP(hipMemsetAsync(buf, 0, (size_t)o.total, (hipStream_t)stream));  // no search yet: every slot 0
    e->stop.stop_at = at<u32>(buf, o.stop_at); e->stop.walked = at<u32>(buf, o.walked);
    e->stop_host_exit = host_exit ? 1 : 0;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_stopped(bz_engine* e, uint32_t* out, void* stream) {
    BZ_REQUIRE(e && out, "bz_engine_stopped: null pointer");
    BZ_REQUIRE(e->stop.stop_at, "bz_engine_stopped: early stop is off (bz_engine_set_early_stop)");
    BZ_HIP(hipMemcpyAsync(out, e->stop.stop_at, (size_t)e->cfg.n_games * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BZ_OK;
}

BZ_EXPORT int32_t bz_early_stop_decided(const uint32_t* N, int32_t n, uint32_t left) {
    if (!(N && n >= 1 && n <= 255)) { set_error("bz_early_stop_decided: null pointer or n outside 1 .. 255"); return -1; }
    for (int i = 0; i < n; ++i)
        if (N[i] >= (1u << 24)) { set_error("bz_early_stop_decided: N[%d] = %u is no visit count (>= 2^24)", i, N[i]); return -1; }
    return early_stop_decided(n, left, [N](int i) { return N[i]; }) ? 1 : 0;
}

/* ---- policy surprise weighting */
namespace {
struct SurpOffsets { int64_t prior, pend, ex_kl, total; };
SurpOffsets surp_carve(const bz_engine_cfg& c) {
    SurpOffsets o{};
    Carver k;
    const int64_t B = c.n_games, maxch = c.game == BZ_GAME_TTT ? TicTacToe::MAXCH : Reversi::MAXCH;
    o.prior = k.take(B * maxch * 4);
    o.pend = k.take(B * 8);
    o.ex_kl = k.take((int64_t)c.rounds * B * c.t_max * 4);
    o.total = k.off;
    return o;
}
}  // namespace

BZ_EXPORT int64_t bz_engine_surprise_bytes(const bz_engine_cfg* cfg) {
    if (!cfg_guard("bz_engine_surprise_bytes", cfg)) return -1;
    return surp_carve(*cfg).total;
}

BZ_EXPORT int32_t bz_engine_set_surprise(bz_engine* e, void* buf, int64_t bytes, void* stream) {
    BZ_REQUIRE(e, "bz_engine_set_surprise: null engine");
    if (!buf) {  // off: no extra launch
        e->surp = SurpDev{};
        return BZ_OK;
    }
    if (option_refusal("bz_engine_set_surprise", BZ_OPT_SURPRISE, e)) return BZ_EINVAL;
    const SurpOffsets o = surp_carve(e->cfg);
    if (int32_t rc = option_buffer("bz_engine_set_surprise", buf, bytes, o.total)) return rc;
    BZ_HIP(hipMemsetAsync(buf, 0, (size_t)o.total, (hipStream_t)stream));  // no prior saved, no row pending, every kl 0
    e->surp.prior = at<float>(buf, o.prior); e->surp.pend = at<u64>(buf, o.pend); e->surp.ex_kl = at<float>(buf, o.ex_kl);
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_pack_surprise(bz_engine* e, float* out, int64_t cap_rows, int32_t append_rows, void* stream) {
    BZ_REQUIRE(e && out, "bz_engine_pack_surprise: null pointer");
    BZ_REQUIRE(e->surp.prior, "bz_engine_pack_surprise: policy surprise weighting is off (bz_engine_set_surprise)");
    BZ_REQUIRE(cap_rows >= 1 && cap_rows <= (int64_t(1) << 31) - 1 && append_rows >= 0 && append_rows <= cap_rows,
               "bz_engine_pack_surprise: bad capacity or append_rows");
    const int n = e->dev.rounds * e->dev.B;
    hipLaunchKernelGGL(k_pack_f32, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, e->dev, e->surp.ex_kl, out, cap_rows);
    BZ_LAUNCH_CHECK("k_pack_f32");
    return BZ_OK;
}

/* ---- search-value targets */
namespace {
int64_t value_bytes(const bz_engine_cfg& c) {
    Carver k;
    k.take((int64_t)c.rounds * c.n_games * c.t_max * 4);
    return k.off;
}
}  // namespace

BZ_EXPORT int64_t bz_engine_search_value_bytes(const bz_engine_cfg* cfg) {
    if (!cfg_guard("bz_engine_search_value_bytes", cfg)) return -1;
    return value_bytes(*cfg);
}

BZ_EXPORT int32_t bz_engine_set_search_value(bz_engine* e, void* buf, int64_t bytes, void* stream) {
    BZ_REQUIRE(e, "bz_engine_set_search_value: null engine");
    if (!buf) {  // off: no extra launch
        e->value = ValueDev{};
        return BZ_OK;
    }
    if (option_refusal("bz_engine_set_search_value", BZ_OPT_SEARCH_VALUE, e)) return BZ_EINVAL;
    const int64_t total = value_bytes(e->cfg);
    if (int32_t rc = option_buffer("bz_engine_set_search_value", buf, bytes, total)) return rc;
    BZ_HIP(hipMemsetAsync(buf, 0, (size_t)total, (hipStream_t)stream));  // every q 0
    e->value.ex_q = static_cast<float*>(buf);
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_pack_search_value(bz_engine* e, float* out, int64_t cap_rows, int32_t append_rows, void* stream) {
    BZ_REQUIRE(e && out, "bz_engine_pack_search_value: null pointer");
    BZ_REQUIRE(e->value.ex_q, "bz_engine_pack_search_value: the search value is not recorded (bz_engine_set_search_value)");
    BZ_REQUIRE(cap_rows >= 1 && cap_rows <= (int64_t(1) << 31) - 1 && append_rows >= 0 && append_rows <= cap_rows,
               "bz_engine_pack_search_value: bad capacity or append_rows");
    const int n = e->dev.rounds * e->dev.B;
    hipLaunchKernelGGL(k_pack_f32, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, e->dev, e->value.ex_q, out, cap_rows);
    BZ_LAUNCH_CHECK("k_pack_f32");
    return BZ_OK;
}

/* ---- ownership targets */
namespace {
struct OwnOffsets { int64_t fin_x, fin_o, pi, act, total; };
OwnOffsets own_carve(const bz_engine_cfg& c) {
    OwnOffsets o{};
    Carver k;
    const int64_t B = c.n_games, na = c.game == BZ_GAME_TTT ? TicTacToe::NA : Reversi::NA;
    o.fin_x = k.take((int64_t)c.rounds * B * 8);
    o.fin_o = k.take((int64_t)c.rounds * B * 8);
    o.pi = k.take(B * na * 4);
    o.act = k.take(B * 4);
    o.total = k.off;
    return o;
}
}  // namespace

BZ_EXPORT int64_t bz_engine_ownership_bytes(const bz_engine_cfg* cfg) {
    if (!cfg_guard("bz_engine_ownership_bytes", cfg)) return -1;
    return own_carve(*cfg).total;
}

BZ_EXPORT int32_t bz_engine_set_ownership(bz_engine* e, void* buf, int64_t bytes, void* stream) {
    BZ_REQUIRE(e, "bz_engine_set_ownership: null engine");
    if (!buf) {  // off: no extra launch
        e->own = OwnDev{};
        return BZ_OK;
    }
    if (option_refusal("bz_engine_set_ownership", BZ_OPT_OWNERSHIP, e)) return BZ_EINVAL;
    const OwnOffsets o = own_carve(e->cfg);
    if (int32_t rc = option_buffer("bz_engine_set_ownership", buf, bytes, o.total)) return rc;
    BZ_HIP(hipMemsetAsync(buf, 0, (size_t)o.total, (hipStream_t)stream));  // no final board; (act 0 is never read before k_root_policy wrote it)
    e->own.fin_x = at<u64>(buf, o.fin_x); e->own.fin_o = at<u64>(buf, o.fin_o);
    e->own.pi = at<float>(buf, o.pi); e->own.act = at<int32_t>(buf, o.act);
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_pack_ownership(bz_engine* e, uint64_t* fown_out, uint64_t* fopp_out, int64_t cap_rows, int32_t append_rows,
                                           void* stream) {
    BZ_REQUIRE(e && fown_out && fopp_out, "bz_engine_pack_ownership: null pointer");
    BZ_REQUIRE(e->own.fin_x, "bz_engine_pack_ownership: the final boards are not recorded (bz_engine_set_ownership)");
    BZ_REQUIRE(cap_rows >= 1 && cap_rows <= (int64_t(1) << 31) - 1 && append_rows >= 0 && append_rows <= cap_rows,
               "bz_engine_pack_ownership: bad capacity or append_rows");
    const int n = e->dev.rounds * e->dev.B;
    hipLaunchKernelGGL(k_pack_own, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, e->dev, e->own,
                       reinterpret_cast<u64*>(fown_out), reinterpret_cast<u64*>(fopp_out), cap_rows);
    BZ_LAUNCH_CHECK("k_pack_own");
    return BZ_OK;
}

/* ---- resignation */
namespace {
struct ResignOffsets { int64_t streak, side, move, q, played_out, total; };
ResignOffsets resign_carve(const bz_engine_cfg& c) {
    ResignOffsets o{};
    Carver k;
    const int64_t n = (int64_t)c.rounds * c.n_games;
    o.streak = k.take(n * 2); o.side = k.take(n); o.move = k.take(n * 4); o.q = k.take(n * 4); o.played_out = k.take(n);
    o.total = k.off;
    return o;
}
}  // namespace

BZ_EXPORT int64_t bz_engine_resign_bytes(const bz_engine_cfg* cfg) {
    if (!cfg_guard("bz_engine_resign_bytes", cfg)) return -1;
    return resign_carve(*cfg).total;
}

BZ_EXPORT int32_t bz_engine_set_resign(bz_engine* e, float threshold, int32_t consecutive, uint32_t playout_q, void* buf, int64_t bytes,
                                       void* stream) {
    if (buf) {  // (what needs no engine first: these refusals can be had without a GPU)
        BZ_REQUIRE(threshold >= -1.0f && threshold <= 1.0f, "bz_engine_set_resign: threshold must be a finite number in [-1, 1]");  // (NaN fails)
        BZ_REQUIRE(consecutive >= 1 && consecutive <= kResignMaxStreak, "bz_engine_set_resign: consecutive must be in 1 .. 255");
        BZ_REQUIRE(playout_q <= 65536u, "bz_engine_set_resign: playout_q must be in 0 .. 65536 (the share of played-out games in units of 2^-16)");
        BZ_REQUIRE((reinterpret_cast<uintptr_t>(buf) & 255) == 0, "bz_engine_set_resign: the buffer must be 256-byte aligned");
    }
    BZ_REQUIRE(e, "bz_engine_set_resign: null engine");
    if (!buf) {  // off: no extra launch
        e->resign = ResignDev{}; e->resign_bytes = 0;
        return BZ_OK;
    }
    if (option_refusal("bz_engine_set_resign", BZ_OPT_RESIGN, e)) return BZ_EINVAL;
    const ResignOffsets o = resign_carve(e->cfg);
    if (int32_t rc = option_buffer("bz_engine_set_resign", buf, bytes, o.total, BZ_EINVAL)) return rc;
    // the buffer the engine already records in: only the rule changes, streaks and records stay
    if (at<uint8_t>(buf, o.streak) != e->resign.streak) BZ_HIP(hipMemsetAsync(buf, 0, (size_t)o.total, (hipStream_t)stream));
    ResignDev& r = e->resign;
    r.threshold = threshold; r.consecutive = consecutive; r.playout_q = playout_q;
    r.streak = at<uint8_t>(buf, o.streak); r.side = at<int8_t>(buf, o.side); r.move = at<int32_t>(buf, o.move);
    r.q = at<float>(buf, o.q); r.played_out = at<uint8_t>(buf, o.played_out);
    e->resign_bytes = o.total;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_resign_rows(bz_engine* e, int8_t* side, int32_t* move, float* q, uint8_t* played_out, void* stream) {
    BZ_REQUIRE(e && side && move && q && played_out, "bz_engine_resign_rows: null pointer");
    BZ_REQUIRE(e->resign.streak, "bz_engine_resign_rows: resignation is off (bz_engine_set_resign)");
    const size_t n = (size_t)e->dev.rounds * e->dev.B;
    hipStream_t s = (hipStream_t)stream;
    BZ_HIP(hipMemcpyAsync(side, e->resign.side, n, hipMemcpyDeviceToDevice, s));
    BZ_HIP(hipMemcpyAsync(move, e->resign.move, n * 4, hipMemcpyDeviceToDevice, s));
    BZ_HIP(hipMemcpyAsync(q, e->resign.q, n * 4, hipMemcpyDeviceToDevice, s));
    BZ_HIP(hipMemcpyAsync(played_out, e->resign.played_out, n, hipMemcpyDeviceToDevice, s));
    return BZ_OK;
}

BZ_EXPORT int32_t bz_resign_step(float q, float threshold, int32_t consecutive, int32_t streak_in, int32_t* streak_out) {
    if (!(streak_out && consecutive >= 1 && consecutive <= kResignMaxStreak && streak_in >= 0 && streak_in <= kResignMaxStreak)) {
        set_error("bz_resign_step: null pointer, consecutive outside 1 .. 255 or streak_in outside 0 .. 255");
        return -1;
    }
    int s;
    const bool fire = resign_step(q, threshold, (int)consecutive, (int)streak_in, &s);
    *streak_out = s;
    return fire ? 1 : 0;
}

BZ_EXPORT int32_t bz_resign_playout(uint64_t seed, uint64_t gid, uint32_t playout_q) {
    if (playout_q > 65536u) { set_error("bz_resign_playout: playout_q must be in 0 .. 65536"); return -1; }
    return resign_played_out((u64)seed, (u64)gid, playout_q) ? 1 : 0;
}

namespace {
struct StoreOffsets { int64_t n_used, idx, hdr, mark, nodes, edges, node_v, tt, total; int n_idx; };
StoreOffsets store_carve(const bz_engine_cfg& c, int64_t S) {
    const Offsets w = carve(c);
    StoreOffsets o{};
    Carver k;
    o.n_idx = 16;
    while ((int64_t)o.n_idx < 2 * S) o.n_idx *= 2;
    o.n_used = k.take(256); o.idx = k.take((int64_t)o.n_idx * 4); o.hdr = k.take(S * (int64_t)sizeof(StoreHdr));
    o.mark = k.take((int64_t)c.n_games * 4);
    o.nodes = k.take(S * w.ncap * (int64_t)sizeof(Node)); o.edges = k.take(S * w.ecap * (int64_t)sizeof(Edge));
    o.node_v = k.take(S * w.ncap * 4); o.tt = k.take(S * w.tt_buckets * 16 * 8);
    o.total = k.off;
    return o;
}
inline bool store_args_ok(int32_t S, int32_t D) { return S >= 1 && S <= 65536 && D >= 1 && D <= 64; }
}  // namespace

/* The root store: bytes of the buffer for `entries` stored searches; 0 for a config whose engine does not run
 * the carry-over cache (the store is off there) */
BZ_EXPORT int64_t bz_engine_root_store_bytes(const bz_engine_cfg* cfg, int32_t entries, int32_t plies) {
    if (!cfg_guard("bz_engine_root_store_bytes", cfg)) return -1;
    if (!store_args_ok(entries, plies)) { set_error("bz_engine_root_store_bytes: 1 <= entries <= 65536, 1 <= plies <= 64"); return -1; }
    if (carve(*cfg).ecache != 2) return 0;
    return store_carve(*cfg, entries).total;
}

BZ_EXPORT int32_t bz_engine_set_root_store(bz_engine* e, void* buf, int64_t bytes, int32_t entries, int32_t plies, void* stream) {
    BZ_REQUIRE(e, "bz_engine_set_root_store: null engine");
    if (!buf || e->dev.ecache != 2) {  // off: no extra launch
        e->store = StoreDev{}; e->store_index_bytes = 0;
        return BZ_OK;
    }
    BZ_REQUIRE(store_args_ok(entries, plies), "bz_engine_set_root_store: 1 <= entries <= 65536, 1 <= plies <= 64");
    if (option_refusal("bz_engine_set_root_store", BZ_OPT_ROOT_STORE, e)) return BZ_EINVAL;
    const StoreOffsets o = store_carve(e->cfg, entries);
    if (int32_t rc = option_buffer("bz_engine_set_root_store", buf, bytes, o.total)) return rc;
    BZ_HIP(hipMemsetAsync(buf, 0, (size_t)o.nodes, (hipStream_t)stream));  // an empty store, no slot seeded
    StoreDev& s = e->store;
    s.S = entries; s.D = plies; s.n_idx = o.n_idx;
    s.base = (e->cfg.game == BZ_GAME_REVERSI && e->cfg.openings) ? 2 : 0;
    s.n_used = at<u32>(buf, o.n_used); s.idx = at<u32>(buf, o.idx); s.hdr = at<StoreHdr>(buf, o.hdr); s.mark = at<u32>(buf, o.mark);
    s.nodes = at<Node>(buf, o.nodes); s.edges = at<Edge>(buf, o.edges); s.node_v = at<float>(buf, o.node_v); s.tt = at<u64>(buf, o.tt);
    e->store_index_bytes = o.mark;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_ownership_row(uint64_t fin_x, uint64_t fin_o, int32_t mover, uint64_t* t_own, uint64_t* t_opp) {
    BZ_REQUIRE(t_own && t_opp && (mover == 1 || mover == -1), "bz_ownership_row: null pointer or mover not +1 / -1");
    u64 a, b;
    ownership_row((u64)fin_x, (u64)fin_o, (int)mover, &a, &b);
    *t_own = a; *t_opp = b;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_root_value(const uint32_t* N, const float* W, int32_t n, float* q) {
    BZ_REQUIRE(N && W && q && n >= 1 && n <= 255, "bz_root_value: null pointer or n outside 1 .. 255");
    *q = root_value(n, [N](int i) { return N[i]; }, [W](int i) { return W[i]; });
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_root_policy(bz_engine* e, float* pi, int32_t* action, void* stream) {
    BZ_REQUIRE(e && pi && action, "bz_engine_root_policy: null pointer");
    const unsigned m = engine_mode(e);
    if (m & kModeForced) {  // 
        BZ_DISPATCH(e, k_forced_root_policy, stream, e->dev, e->cap, e->forced, pi, action);
        return BZ_OK;
    }
    BZ_DISPATCH(e, k_root_policy, stream, e->dev, e->gumbel, (m & kModeSolve) ? 1 : 0, pi, action);
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_reanalyse_load(bz_engine* e, const uint64_t* own, const uint64_t* opp, const int8_t* mover, int64_t n_rows,
                                           const int64_t* rows, int64_t first, int32_t count, int32_t clear, void* stream) {
    BZ_REQUIRE(e && own && opp && mover, "bz_engine_reanalyse_load: null pointer");
    BZ_REQUIRE(count >= 0 && count <= e->dev.B, "bz_engine_reanalyse_load: count outside 0 .. n_games");
    BZ_REQUIRE(first >= 0 && n_rows >= 0, "bz_engine_reanalyse_load: negative first or n_rows");
    BZ_DISPATCH(e, k_reanalyse_load, stream, e->dev, own, opp, mover, n_rows, rows, first, (int)count, (int)(clear != 0));
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_reanalyse_store(bz_engine* e, float* pi, float* q, float* kl, int64_t n_rows, const int64_t* rows,
                                            int64_t first, int32_t count, void* stream) {
    BZ_REQUIRE(e && pi, "bz_engine_reanalyse_store: null pointer");
    BZ_REQUIRE(count >= 0 && count <= e->dev.B, "bz_engine_reanalyse_store: count outside 0 .. n_games");
    BZ_REQUIRE(first >= 0 && n_rows >= 0, "bz_engine_reanalyse_store: negative first or n_rows");
    if (count == 0) return BZ_OK;
    const unsigned m = engine_mode(e);
    const dim3 grid((count + 63) / 64);  // (one lane per slot, 64 slots per block)
#define BZ_RSTORE(G) \
    hipLaunchKernelGGL(k_reanalyse_store<G>, grid, dim3(64), 0, (hipStream_t)stream, e->dev, e->gumbel, e->forced, \
                       (m & kModeForced) ? 1 : 0, (m & kModeSolve) ? 1 : 0, pi, q, kl, n_rows, rows, first, (int)count)
    switch (e->cfg.game) {
    case BZ_GAME_TTT: BZ_RSTORE(TicTacToe); break;
    case BZ_GAME_REVERSI6: BZ_RSTORE(Reversi6); break;
    case BZ_GAME_REVERSI4: BZ_RSTORE(Reversi4); break;
    default: BZ_RSTORE(Reversi); break;
    }
#undef BZ_RSTORE
    BZ_LAUNCH_CHECK("k_reanalyse_store");
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_play(bz_engine* e, int32_t restart, void* stream) {
    BZ_REQUIRE(e, "null engine");
    if (e->resign.streak)  //  first: a slot that resigns here is out of every kernel below
        BZ_DISPATCH(e, k_resign_note, stream, e->dev, e->resign, cap_budgets(e));
    if (e->surp.prior) {  //  the row this play is about to write
        // without Dirichlet noise the searched root still holds its raw priors (only the noise ever rewrites a prior): saved here,
        // whichever way the search ran -- fused, step kernels, the step API
        if (!(e->dev.dir_eps > 0.0f)) BZ_DISPATCH(e, k_surp_save, stream, e->dev, e->surp);
        hipLaunchKernelGGL(k_surp_note, grid_of(e->dev.B), dim3(256), 0, (hipStream_t)stream, e->dev, e->surp,
                           cap_budgets(e));
        BZ_LAUNCH_CHECK("k_surp_note");
    }
    if (e->value.ex_q) {  //  the root's search value of the row this play is about to write
        hipLaunchKernelGGL(k_root_q, grid_of(e->dev.B), dim3(256), 0, (hipStream_t)stream, e->dev, e->value,
                           cap_budgets(e));
        BZ_LAUNCH_CHECK("k_root_q");
    }
    if (e->own.fin_x) {  //  the final board of every game this play ends, while the root it plays from is in place
        int32_t rc = bz_engine_root_policy(e, e->own.pi, e->own.act, stream);
        if (rc != BZ_OK) return rc;
        BZ_DISPATCH(e, k_own_final, stream, e->dev, e->own, cap_budgets(e));
    }
    {
        ProfScope ps(BZ_PROF_PLAY, stream);
        // the move does not depend on how the walks ran: leaf-parallel, FPU and the interior rule play as their base mode does
        const unsigned m = engine_mode(e) & ~(kModeLeaf | kModeFpu | kModeGfull);
#define BZ_PLAY(KERNEL, ...) BZ_DISPATCH(e, KERNEL, stream, __VA_ARGS__, (int)restart); break
        switch (m) {
        case 0u: BZ_PLAY(k_play, e->dev);
        case kModeGumbel: BZ_PLAY(k_gumbel_play, e->dev, e->gumbel);  // 
        case kModeCap: BZ_PLAY(k_cap_play, e->dev, e->cap);  // 
        case kModeForced: BZ_PLAY(k_forced_play, e->dev, e->forced);  // 
        case kModeForced | kModeCap: BZ_PLAY(k_forced_cap_play, e->dev, e->cap, e->forced);
        case kModeSolve: BZ_PLAY(k_solve_play, e->dev);  // 
        case kModeSolve | kModeCap: BZ_PLAY(k_solve_cap_play, e->dev, e->cap);
        case kModeStop: BZ_PLAY(k_play, e->dev);  //  a stopped search is a full search: the plain move over the tree as it stands
        default: set_error("bz_engine_play: no play kernel serves search mode 0x%x", m); return BZ_EINVAL;
        }
#undef BZ_PLAY
    }
    if (e->surp.prior) BZ_DISPATCH(e, k_surp_kl, stream, e->dev, e->surp);  // ... and its kl (before the arenas swap below)
    if (e->resign.streak) BZ_DISPATCH(e, k_resign_finish, stream, e->dev, (int)restart);  // 
    if (e->dev.reuse) {  // the tree just searched becomes the source of the next root_begin's subtree copy
        Node* tn = e->dev.nodes; e->dev.nodes = e->dev.nodes_alt; e->dev.nodes_alt = tn;
        Edge* te = e->dev.edges; e->dev.edges = e->dev.edges_alt; e->dev.edges_alt = te;
    }
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engine_status(bz_engine* e, void* stream, int32_t* n_active, int64_t* games_finished,
                                   int32_t* error_flags) {
    BZ_REQUIRE(e, "null engine");
    hipStream_t s = (hipStream_t)stream;
    BZ_HIP(hipMemsetAsync(e->dev.flags + FLAG_ACTIVE, 0, 4, s));
    hipLaunchKernelGGL(k_count_active, grid_of(e->dev.B), dim3(256), 0, s, e->dev);
    BZ_LAUNCH_CHECK("k_count_active");
    u32 h[FLAG_N];
    BZ_HIP(hipMemcpyAsync(h, e->dev.flags, sizeof(h), hipMemcpyDeviceToHost, s));
    BZ_HIP(hipStreamSynchronize(s));
    if (n_active) *n_active = (int32_t)h[FLAG_ACTIVE];
    if (games_finished) *games_finished = (int64_t)h[FLAG_FINISHED];
    if (error_flags) *error_flags = (int32_t)h[FLAG_ERR];
    return BZ_OK;
}



namespace {
PackedLayout packed_layout(int na, int64_t cap) {
    PackedLayout L{};
    Carver k;
    k.take(256);  // header first: a prefix of the block describes the rest
    const int64_t esz[8] = {8, 8, 4 * (int64_t)na, 8, 1, 1, 1, 1};
    for (int i = 0; i < 8; ++i) L.offs[i] = k.take(cap * esz[i]);
    L.total = k.off;
    return L;
}
}  // namespace

BZ_EXPORT int64_t bz_examples_packed_bytes(int32_t na, int64_t cap_rows) {
    if (na < 1 || na > 4096 || cap_rows < 1 || cap_rows > (int64_t(1) << 31) - 1) { set_error("bz_examples_packed_bytes: bad arguments"); return -1; }
    return packed_layout(na, cap_rows).total;
}

/* compact the finished games' rows of this engine into the caller's packed block (append != 0: behind the rows a
 * previous call -- another engine of the same geometry -- left there) */
BZ_EXPORT int32_t bz_engine_pack_examples(bz_engine* e, void* packed, int64_t packed_bytes, int64_t cap_rows, int32_t append,
                                          void* stream) {
    BZ_REQUIRE(e && packed, "bz_engine_pack_examples: null pointer");
    BZ_REQUIRE(cap_rows >= 1 && cap_rows <= (int64_t(1) << 31) - 1, "bz_engine_pack_examples: bad capacity");
    BZ_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 255) == 0, "bz_engine_pack_examples: the block must be 256-byte aligned");
    const PackedLayout L = packed_layout(e->dev.na, cap_rows);
    if (packed_bytes < L.total) { set_error("bz_engine_pack_examples: block too small (%lld < %lld)", (long long)packed_bytes, (long long)L.total); return BZ_ENOMEM; }
    hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(1024), 0, (hipStream_t)stream, e->dev, static_cast<PackedHdr*>(packed), L,
                       (u64)cap_rows, (int)(append != 0), (int)e->cfg.game);
    BZ_LAUNCH_CHECK("k_pack_scan");
    const int n = e->dev.rounds * e->dev.B;
    hipLaunchKernelGGL(k_pack_rows, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, e->dev, static_cast<char*>(packed), L);
    BZ_LAUNCH_CHECK("k_pack_rows");
    return BZ_OK;
}

/* names used by SURVEY.md 8(b) for the same entry points */
BZ_EXPORT int32_t bz_mcts_select(bz_engine* e, uint32_t sim_index, void* stream) { return bz_engine_select(e, sim_index, stream); }
BZ_EXPORT int32_t bz_mcts_expand_backup(bz_engine* e, void* stream) { return bz_engine_expand_backup(e, stream); }
/* one move for every active slot: search (root expansion + cfg.sims simulations) then play */
BZ_EXPORT int32_t bz_selfplay_run(bz_engine* e, int32_t restart, void* stream) {
    int32_t rc = bz_engine_search(e, stream);
    return rc != BZ_OK ? rc : bz_engine_play(e, restart, stream);
}

/* One move (search + play) for several engines at once -- the pipelines of one GPU, each on its own stream -- issued
 * by ONE host thread, interleaved simulation by simulation, so that every stream always has work queued whatever the
 * host's run-ahead.  run_ahead_sims > 0 bounds that run-ahead: every run_ahead_sims / 2 simulations the thread records
 * a blocking-sync event per stream and sleeps on the one recorded two marks earlier.  Without the bound the thread
 * queues launches until the runtime's queue is full and then spins there: measured 100 % of a core for the whole
 * timed region (plus a second runtime thread), which eight ranks on one host cannot afford. */
static int32_t ahead_mark(bz_engine* e, int idx, hipStream_t s) {
    while (e->n_ahead < 4) {
        BZ_HIP(hipEventCreateWithFlags(&e->ahead[e->n_ahead], hipEventBlockingSync | hipEventDisableTiming));
        e->n_ahead++;
    }
    BZ_HIP(hipEventRecord(e->ahead[idx & 3], s));
    if (idx >= 2) {
        // hipEventSynchronize spins on this stack even for hipEventBlockingSync events (measured: the thread stayed at
        // 100 % of a core), so the wait is a poll with real sleeps; a mark is many milliseconds of queued GPU work
        const timespec nap = {0, 100 * 1000};
        for (;;) {
            const hipError_t q = hipEventQuery(e->ahead[(idx - 2) & 3]);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return hip_fail(q, "bz_engines_step: hipEventQuery");
            (void)hipGetLastError();  // hipErrorNotReady is sticky in hipGetLastError
            nanosleep(&nap, nullptr);
        }
    }
    return BZ_OK;
}

// the body of bz_engines_step / bz_engines_search: one search per (non-null) engine, the stepwise ones interleaved tree
// step by tree step -- each with its own sims, K and mode -- and, with `play`, the move behind each
static int32_t engines_run(bz_engine* const* engines, void* const* streams, int n, int run_ahead_sims, bool play, int restart) {
    int32_t rc;
    int steps = 0, Kmax = 1;
    for (int i = 0; i < n; ++i) {
        bz_engine* e = engines[i];
        if (!e || search_is_fused(e)) continue;
        const int ns = (e->cfg.sims + e->dev.K - 1) / e->dev.K;
        steps = ns > steps ? ns : steps;
        Kmax = e->dev.K > Kmax ? e->dev.K : Kmax;
        if ((rc = bz_engine_root_begin(e, streams[i])) != BZ_OK) return rc;
        if ((rc = paced_search(e, streams[i])) != BZ_OK) return rc;
        if ((rc = bz_engine_evaluate(e, streams[i])) != BZ_OK) return rc;
        if (root_prep(e)) {
            if ((rc = tree_step(e, 1, 0, 0, streams[i])) != BZ_OK) return rc;
            if ((rc = bz_engine_root_noise(e, streams[i])) != BZ_OK) return rc;
        }
    }
    for (int i = 0; i < n; ++i) {  // (behind the stepwise engines' root launches, so that those streams have work first)
        bz_engine* e = engines[i];
        if (!e || !search_is_fused(e)) continue;
        if ((rc = bz_engine_search(e, streams[i])) != BZ_OK) return rc;
        if (play && (rc = bz_engine_play(e, restart, streams[i])) != BZ_OK) return rc;
    }
    // (K > 1: one step = K simulations; the run-ahead bound counts steps of q / K, at least one)
    const int q0 = run_ahead_sims > 0 ? (run_ahead_sims >= 2 ? run_ahead_sims / 2 : 1) : 0;
    const int q = q0 ? (q0 / Kmax > 0 ? q0 / Kmax : 1) : 0;
    //  host exit: an engine with early stop whose slots have all stopped walking leaves the loop.  It learns that
    // from the marks it waits on anyway: in front of every mark's event its stream copies stop.walked (1 + the last step in which
    // a slot walked) into a pinned word, and the mark found complete -- the one after step m -- with walked <= m says step m was
    // empty.  A slot that does not walk is left LEAF_NONE and never walks again, so every later step is empty too.
    bool quit[16] = {};  // (n <= 16)
    for (int step = 0; step < steps; ++step) {
        int live = 0;
        for (int i = 0; i < n; ++i) {
            bz_engine* e = engines[i];
            if (!e || search_is_fused(e) || quit[i]) continue;
            const int s = step * e->dev.K;
            if (s >= e->cfg.sims) continue;
            ++live;
            const bool prep = root_prep(e);
            if ((rc = tree_step(e, (prep && s == 0) ? 0 : 1, 1, (uint32_t)s, streams[i])) != BZ_OK) return rc;
            if ((rc = bz_engine_evaluate(e, streams[i])) != BZ_OK) return rc;
        }
        if (!live) break;
        if (q && (step + 1) % q == 0)
            for (int i = 0; i < n; ++i) {
                bz_engine* e = engines[i];
                if (!e || search_is_fused(e) || quit[i]) continue;
                const int idx = (step + 1) / q - 1;
                const bool watch = !play && e->stop.stop_at && e->stop_host_exit;  // (bz_engines_search only)
                if (watch) {
                    if (!e->stop_ring) BZ_HIP(hipHostMalloc(reinterpret_cast<void**>(&e->stop_ring), 4 * sizeof(uint32_t), hipHostMallocDefault));
                    BZ_HIP(hipMemcpyAsync(e->stop_ring + (idx & 3), e->stop.walked, 4, hipMemcpyDeviceToHost, (hipStream_t)streams[i]));
                }
                if ((rc = ahead_mark(e, idx, (hipStream_t)streams[i])) != BZ_OK) return rc;
                // (mark idx - 2 is complete, and it was recorded behind step (idx - 1) * q - 1)
                if (watch && idx >= 2 && (int)e->stop_ring[(idx - 2) & 3] <= (idx - 1) * q - 1) quit[i] = true;
            }
    }
    for (int i = 0; i < n; ++i) {
        bz_engine* e = engines[i];
        if (!e || search_is_fused(e)) continue;
        if ((rc = tree_step(e, 1, 0, 0, streams[i])) != BZ_OK) return rc;
        e->seed_from_prev = e->paced;
        if ((rc = store_save(e, streams[i])) != BZ_OK) return rc;
        if (play && (rc = bz_engine_play(e, restart, streams[i])) != BZ_OK) return rc;
    }
    return BZ_OK;
}

BZ_EXPORT int32_t bz_engines_step(bz_engine* const* engines, void* const* streams, int32_t n, int32_t restart,
                                  int32_t run_ahead_sims) {
    BZ_REQUIRE(engines && streams && n >= 1 && n <= 16 && run_ahead_sims >= 0, "bz_engines_step: bad arguments");
    bool stepwise = true;
    for (int i = 0; i < n; ++i) {
        BZ_REQUIRE(engines[i], "bz_engines_step: null engine");
        BZ_REQUIRE(engines[i]->cfg.sims == engines[0]->cfg.sims, "bz_engines_step: the engines must search the same number of simulations");
        BZ_REQUIRE(engines[i]->dev.K == engines[0]->dev.K, "bz_engines_step: the engines must take the same leaves per step");
        BZ_REQUIRE((engines[i]->gumbel.m > 0) == (engines[0]->gumbel.m > 0),
                   "bz_engines_step: the engines must all search with Gumbel root search or all without");
        BZ_REQUIRE((engines[i]->gin.node_v != nullptr) == (engines[0]->gin.node_v != nullptr),
                   "bz_engines_step: the engines must all search with the Gumbel interior rule or all without");
        BZ_REQUIRE(engines[i]->cfg.eval_kind != BZ_EVAL_EXTERNAL, "bz_engines_step: BZ_EVAL_EXTERNAL callers drive the step API");
        if (search_is_fused(engines[i])) stepwise = false;
    }
    if (!stepwise) {  // a fused search is one launch per engine: nothing to interleave
        int32_t rc;
        for (int i = 0; i < n; ++i)
            if ((rc = bz_selfplay_run(engines[i], restart, streams[i])) != BZ_OK) return rc;
        return BZ_OK;
    }
    return engines_run(engines, streams, n, run_ahead_sims, true, restart);
}

BZ_EXPORT int32_t bz_engines_search(bz_engine* const* engines, void* const* streams, int32_t n, int32_t run_ahead_sims) {
    BZ_REQUIRE(engines && streams && n >= 1 && n <= 16 && run_ahead_sims >= 0, "bz_engines_search: bad arguments");
    for (int i = 0; i < n; ++i)
        BZ_REQUIRE(!engines[i] || engines[i]->cfg.eval_kind != BZ_EVAL_EXTERNAL,
                   "bz_engines_search: BZ_EVAL_EXTERNAL callers drive the step API");
    return engines_run(engines, streams, n, run_ahead_sims, false, 0);
}

// the engine's sticky error word (FLAG_ERR: BZ_ENGINE_ERR_* bits) in device memory -- bz_match.hip's ply kernel folds it
// into the match header, so that a match needs no bz_engine_status round trip per ply
const uint32_t* bz_engine_error_word_dev(const bz_engine* e) { return e->dev.flags + FLAG_ERR; }
