// bz_match.hip -- the driver of a head-to-head match between two search players: everything that
// happens to B concurrent games BETWEEN two searches, as one kernel per ply.
//
// A match is two bz_engines over the same B game slots, one per side (A and B).  Per ply the host sets each engine's
// roots, searches the engines that have a slot to move, asks both for their moves (bz_engine_root_policy) and launches
// k_match_ply: one lane per game takes the action of the side to move (or the opening move), applies it through the rule
// functions of bz_rules.h, handles terminal positions and the pass rule (the turn loop of ReversiTerminal.play,
// reversi_terminal.py:16-38, resp. TicTacToeHeadless.play, tic_tac_toe.py:13-34, as the arena implements it), logs the
// move and writes the NEXT ply's roots for both engines plus a 32-byte header the host reads once per ply.
//
// Every active slot makes exactly one move per ply (a pass is no ply: the same side moves again), so the number of
// moves a slot has made equals the ply index while it is active; the log is [max_plies][B].
//
// Games 2k and 2k+1 are a pair: the same opening, A plays X (+1, moves first) in 2k and O in 2k+1.  Opening move at ply
// t < opening_plies: the r-th legal move in ascending action order, r = rng_draw(seed ^ kMatchSeed, k, t) mod n_legal.
#include <new>

#include "bz_common.h"
#include "bz_math.h"
#include "bz_rules.h"

using namespace bz;

// bz_mcts.hip: the engine's sticky error word (BZ_ENGINE_ERR_* bits) in device memory
const uint32_t* bz_engine_error_word_dev(const bz_engine* e);

namespace {

constexpr u64 kMatchSeed = 0x6D617463684F50E5ULL;  // C_MATCH of DESIGN.md 3.14
constexpr int kHdrWords = 8;                       // u32 per header row
enum { HDR_ACTIVE = 0, HDR_TO_MOVE_A = 1, HDR_TO_MOVE_B = 2, HDR_ERROR = 3, HDR_ENGINE_ERR_A = 4, HDR_ENGINE_ERR_B = 5 };
enum { SLOT_FINISHED = 0, SLOT_ACTIVE = 1, SLOT_FROZEN = 2 };

BZ_HD u32 opening_index(u64 seed, u64 pair, u64 ply, u32 n_legal) {
    return (u32)(rng_draw(seed ^ kMatchSeed, pair, ply) % (u64)n_legal);
}

struct MatchDev {
    u64 *own, *opp;          // [B] position seen by the side to move: the roots of BOTH engines
    int8_t *to_move;         // [B] absolute colour of the side to move
    uint8_t* active;         // [B] SLOT_*
    int8_t *winner;          // [B] absolute colour, valid once the slot is finished
    int32_t* plies;          // [B] moves made
    int8_t* a_colour;        // [B] the colour side A plays
    int8_t *tm_a, *tm_b;     // [B] to_move of the next search's roots per engine (0 = slot idle in that engine)
    uint8_t* log_action;     // [max_plies][B], 255 = no move by this slot at this ply
    int8_t* log_mover;       // [max_plies][B], 0 = no move
    u32* hdr;                // [max_plies + 1][kHdrWords]: row t = the state BEFORE ply t
    int B, max_plies, opening_plies;
    u64 seed;
};

// the r-th set bit of m (r < popcount(m))
__device__ __forceinline__ int nth_bit(u64 m, u32 r) {
    for (u32 j = 0; j < r; ++j) m &= m - 1;
    return ctz64(m);
}

// counts of this ply's outcome into the next header row: one atomic per wave and word
__device__ __forceinline__ void count_into(u32* word, bool flag) {
    const unsigned long long b = __ballot(flag);
    if (b != 0 && (threadIdx.x & (warpSize - 1)) == (unsigned)ctz64((u64)b)) atomicAdd(word, (u32)popc64((u64)b));
}

__device__ __forceinline__ void write_roots(const MatchDev& M, int g, bool act, int tm, int ac, int plies, u32* next) {
    const bool searched = act && plies >= M.opening_plies;
    const bool a_moves = searched && tm == ac, b_moves = searched && tm != ac;
    M.tm_a[g] = (int8_t)(a_moves ? tm : 0);
    M.tm_b[g] = (int8_t)(b_moves ? tm : 0);
    count_into(next + HDR_ACTIVE, act);
    count_into(next + HDR_TO_MOVE_A, a_moves);
    count_into(next + HDR_TO_MOVE_B, b_moves);
}

template <class G>
__global__ void __launch_bounds__(256) k_match_begin(MatchDev M) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = g < M.B;
    if (in) {
        u64 own, opp;
        G::start(&own, &opp);
        const int ac = (g & 1) ? -1 : 1;
        M.own[g] = own; M.opp[g] = opp; M.to_move[g] = 1; M.active[g] = SLOT_ACTIVE; M.winner[g] = 0; M.plies[g] = 0;
        M.a_colour[g] = (int8_t)ac;
        write_roots(M, g, true, 1, ac, 0, M.hdr);
    }
}

// one ply of every game.  act_a / act_b: the engines' moves, i32 [B], -1 = that engine searched nothing for the slot.
// err_a / err_b (may be null): the engines' error words, folded into the header so that the host's one read sees them.
template <class G>
__global__ void __launch_bounds__(256) k_match_ply(MatchDev M, const int32_t* __restrict__ act_a, const int32_t* __restrict__ act_b,
                                                   const u32* __restrict__ err_a, const u32* __restrict__ err_b, int ply) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const u32* cur = M.hdr + (size_t)ply * kHdrWords;
    u32* next = M.hdr + (size_t)(ply + 1) * kHdrWords;
    const u32 prev_err = cur[HDR_ERROR];
    if (g == 0) {  // the sticky words travel from row to row (nobody else writes HDR_ERROR once it is set)
        if (prev_err) next[HDR_ERROR] = prev_err;
        next[HDR_ENGINE_ERR_A] = cur[HDR_ENGINE_ERR_A] | (err_a ? *err_a : 0u);
        next[HDR_ENGINE_ERR_B] = cur[HDR_ENGINE_ERR_B] | (err_b ? *err_b : 0u);
    }
    const bool in = g < M.B;
    bool act = false;
    int tm = 0, ac = 0, plies = 0;
    if (in && M.active[g] == SLOT_ACTIVE) {
        u64 own = M.own[g], opp = M.opp[g];
        tm = M.to_move[g]; ac = M.a_colour[g]; plies = M.plies[g];
        const u64 legal = G::legal(own, opp);
        int a;
        if (plies < M.opening_plies) a = legal ? nth_bit(legal, opening_index(M.seed, (u64)(g >> 1), (u64)plies, (u32)popc64(legal))) : -1;
        else a = tm == ac ? act_a[g] : act_b[g];
        constexpr int kCells = G::NA == 65 ? 64 : G::NA;  // (Reversi's action 64, the pass, exists only inside the search tree)
        if (a < 0 || a >= kCells || !((legal >> a) & 1ULL)) {
            // refused: the slot is frozen as it stands, the first such slot is named in the error word
            M.active[g] = SLOT_FROZEN;
            if (!prev_err) atomicCAS(next + HDR_ERROR, 0u, (a < 0 ? BZ_MATCH_ERR_NO_ACTION : BZ_MATCH_ERR_ILLEGAL) | (u32)g);
        } else {
            u64 cown, copp;  // the position after the move, seen by the other side
            G::apply(own, opp, a, &cown, &copp);
            M.log_action[(size_t)ply * M.B + g] = (uint8_t)a;
            M.log_mover[(size_t)ply * M.B + g] = (int8_t)tm;
            plies++;
            M.plies[g] = plies;
            const u64 lnext = G::legal(cown, copp);
            int tv;
            if (G::terminal(cown, copp, -tm, lnext, &tv)) {
                M.winner[g] = (int8_t)(tv * -tm);
                M.active[g] = SLOT_FINISHED;
                M.own[g] = cown; M.opp[g] = copp; M.to_move[g] = (int8_t)-tm;
            } else {
                act = true;
                if (lnext == 0) { M.own[g] = copp; M.opp[g] = cown; }  // the other side has no move: the same side moves again
                else { M.own[g] = cown; M.opp[g] = copp; tm = -tm; M.to_move[g] = (int8_t)tm; }
            }
        }
    }
    if (in && !act) { M.tm_a[g] = 0; M.tm_b[g] = 0; }
    if (in && act) write_roots(M, g, true, tm, ac, plies, next);
}

struct Offsets { int64_t own, opp, to_move, active, winner, plies, a_colour, tm_a, tm_b, log_action, log_mover, hdr, total; };

Offsets carve(int B, int T) {
    Offsets o;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { int64_t at = off; off += (bytes + 255) & ~(int64_t)255; return at; };
    o.own = take(8LL * B); o.opp = take(8LL * B); o.to_move = take(B); o.active = take(B); o.winner = take(B);
    o.plies = take(4LL * B); o.a_colour = take(B); o.tm_a = take(B); o.tm_b = take(B);
    o.log_action = take((int64_t)T * B); o.log_mover = take((int64_t)T * B);
    o.hdr = take(4LL * kHdrWords * (T + 1));
    o.total = off;
    return o;
}

int game_plies(int game) {  // the longest game: every empty cell of the start position filled
    switch (game) {
    case BZ_GAME_TTT: return 9;
    case BZ_GAME_REVERSI: return 60;
    case BZ_GAME_REVERSI6: return 32;
    case BZ_GAME_REVERSI4: return 12;
    default: return -1;
    }
}

const char* args_bad(int game, int n_games, int max_plies) {
    if (game_plies(game) < 0) return "unknown game";
    if (n_games < 2 || (n_games & 1) || n_games > BZ_MATCH_MAX_GAMES) return "n_games must be even, 2 .. BZ_MATCH_MAX_GAMES (games 2k and 2k+1 are a pair)";
    if (max_plies < 0 || max_plies > 64) return "max_plies must be in 1..64, or 0 = the game's longest game";
    return nullptr;
}

}  // namespace

struct bz_match {
    MatchDev dev;
    Offsets off;
    int game, ply;
    bool begun;
};

#define BZ_MATCH_LAUNCH(m, KERNEL, stream, ...)                                                                         \
    do {                                                                                                                \
        const dim3 grid_((unsigned)(((m)->dev.B + 255) / 256));                                                         \
        switch ((m)->game) {                                                                                            \
        case BZ_GAME_TTT: hipLaunchKernelGGL((KERNEL<TicTacToe>), grid_, dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__); break; \
        case BZ_GAME_REVERSI6: hipLaunchKernelGGL((KERNEL<Reversi6>), grid_, dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__); break; \
        case BZ_GAME_REVERSI4: hipLaunchKernelGGL((KERNEL<Reversi4>), grid_, dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((KERNEL<Reversi>), grid_, dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__); break;  \
        }                                                                                                               \
        BZ_LAUNCH_CHECK(#KERNEL);                                                                                       \
    } while (0)

BZ_EXPORT int32_t bz_match_opening_index(uint64_t seed, uint64_t pair, int32_t ply, int32_t n_legal, int32_t* index) {
    BZ_REQUIRE(index && ply >= 0 && n_legal >= 1 && n_legal <= 64, "bz_match_opening_index: ply >= 0 and 1 <= n_legal <= 64");
    *index = (int32_t)opening_index(seed, pair, (u64)ply, (u32)n_legal);
    return BZ_OK;
}

BZ_EXPORT int64_t bz_match_workspace_bytes(int32_t game, int32_t n_games, int32_t max_plies) {
    if (const char* why = args_bad(game, n_games, max_plies)) { set_error("bz_match_workspace_bytes: %s", why); return -1; }
    return carve(n_games, max_plies ? max_plies : game_plies(game)).total;
}

BZ_EXPORT int32_t bz_match_create(int32_t game, int32_t n_games, int32_t max_plies, void* ws, int64_t bytes, bz_match** out) {
    BZ_REQUIRE(ws && out, "bz_match_create: null pointer");
    if (const char* why = args_bad(game, n_games, max_plies)) { set_error("bz_match_create: %s", why); return BZ_EINVAL; }
    if (bz_device_count() <= 0) { set_error("bz_match_create: no HIP device (the match has no CPU path)"); return BZ_ENOGPU; }
    if (max_plies == 0) max_plies = game_plies(game);
    const Offsets o = carve(n_games, max_plies);
    if (bytes < o.total) { set_error("bz_match_create: workspace too small (%lld < %lld)", (long long)bytes, (long long)o.total); return BZ_ENOMEM; }
    BZ_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "bz_match_create: workspace must be 256-byte aligned");
    bz_match* m = new (std::nothrow) bz_match();
    if (!m) { set_error("out of host memory"); return BZ_ENOMEM; }
    char* p = static_cast<char*>(ws);
    MatchDev& d = m->dev;
    d.own = (u64*)(p + o.own); d.opp = (u64*)(p + o.opp); d.to_move = (int8_t*)(p + o.to_move); d.active = (uint8_t*)(p + o.active);
    d.winner = (int8_t*)(p + o.winner); d.plies = (int32_t*)(p + o.plies); d.a_colour = (int8_t*)(p + o.a_colour);
    d.tm_a = (int8_t*)(p + o.tm_a); d.tm_b = (int8_t*)(p + o.tm_b); d.log_action = (uint8_t*)(p + o.log_action);
    d.log_mover = (int8_t*)(p + o.log_mover); d.hdr = (u32*)(p + o.hdr);
    d.B = n_games; d.max_plies = max_plies; d.opening_plies = 0; d.seed = 0;
    m->off = o; m->game = game; m->ply = 0; m->begun = false;
    *out = m;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_match_destroy(bz_match* m) {
    delete m;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_match_get_layout(const bz_match* m, bz_match_layout* out) {
    BZ_REQUIRE(m && out, "bz_match_get_layout: null pointer");
    const Offsets& o = m->off;
    out->own = o.own; out->opp = o.opp; out->to_move = o.to_move; out->active = o.active; out->winner = o.winner;
    out->plies = o.plies; out->a_colour = o.a_colour; out->to_move_a = o.tm_a; out->to_move_b = o.tm_b;
    out->log_action = o.log_action; out->log_mover = o.log_mover;
    out->n_games = m->dev.B; out->max_plies = m->dev.max_plies;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_match_begin(bz_match* m, uint64_t seed, int32_t opening_plies, void* stream) {
    BZ_REQUIRE(m, "bz_match_begin: null match");
    BZ_REQUIRE(opening_plies >= 0, "bz_match_begin: opening_plies must be >= 0");
    hipStream_t s = (hipStream_t)stream;
    MatchDev& d = m->dev;
    d.seed = seed; d.opening_plies = opening_plies;
    const size_t log_bytes = (size_t)d.max_plies * d.B;
    BZ_HIP(hipMemsetAsync(d.log_action, 0xFF, log_bytes, s));
    BZ_HIP(hipMemsetAsync(d.log_mover, 0, log_bytes, s));
    BZ_HIP(hipMemsetAsync(d.hdr, 0, sizeof(u32) * kHdrWords * (size_t)(d.max_plies + 1), s));
    BZ_MATCH_LAUNCH(m, k_match_begin, s, d);
    m->ply = 0; m->begun = true;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_match_ply(bz_match* m, const int32_t* action_a, const int32_t* action_b, const bz_engine* engine_a,
                               const bz_engine* engine_b, void* stream) {
    BZ_REQUIRE(m && action_a && action_b, "bz_match_ply: null pointer");
    if (!m->begun) { set_error("bz_match_ply: bz_match_begin first"); return BZ_ESTATE; }
    if (m->ply >= m->dev.max_plies) { set_error("bz_match_ply: the match has played its max_plies (%d) plies", m->dev.max_plies); return BZ_ESTATE; }
    const u32* ea = engine_a ? bz_engine_error_word_dev(engine_a) : nullptr;
    const u32* eb = engine_b ? bz_engine_error_word_dev(engine_b) : nullptr;
    BZ_MATCH_LAUNCH(m, k_match_ply, stream, m->dev, action_a, action_b, ea, eb, m->ply);
    m->ply++;
    return BZ_OK;
}

BZ_EXPORT int32_t bz_match_header(bz_match* m, void* stream, bz_match_hdr* out) {
    BZ_REQUIRE(m && out, "bz_match_header: null pointer");
    if (!m->begun) { set_error("bz_match_header: bz_match_begin first"); return BZ_ESTATE; }
    hipStream_t s = (hipStream_t)stream;
    u32 h[kHdrWords];
    BZ_HIP(hipMemcpyAsync(h, m->dev.hdr + (size_t)m->ply * kHdrWords, sizeof(h), hipMemcpyDeviceToHost, s));
    BZ_HIP(hipStreamSynchronize(s));
    out->ply = m->ply; out->n_active = (int32_t)h[HDR_ACTIVE]; out->n_to_move_a = (int32_t)h[HDR_TO_MOVE_A];
    out->n_to_move_b = (int32_t)h[HDR_TO_MOVE_B]; out->error = h[HDR_ERROR]; out->engine_err_a = h[HDR_ENGINE_ERR_A];
    out->engine_err_b = h[HDR_ENGINE_ERR_B]; out->reserved = 0;
    return BZ_OK;
}
