/*
 * bz_abi.h -- C ABI of libbz_hip.so, the MI355X (gfx950) self-play engine that
 * drops in behind BetaZero's Python Game / Player API.
 *
 * The reference (whaiproject/BetaZero) is pure Python and has NO FFI: the seams
 * this ABI sits behind are duck-typed Python interfaces.  Each entry point
 * cites the reference interface it replaces (paths relative to the reference
 * root).  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *  - extern "C", plain C types only; every function returns int32_t status
 *    (BZ_OK or a BZ_E* code) and never throws / aborts; bz_last_error() gives
 *    the thread-local message of the last failure.
 *  - Batched entry points take RAW DEVICE POINTERS (torch.Tensor.data_ptr()),
 *    element counts and a hipStream_t passed as void* (0 = default stream).
 *    They are asynchronous on that stream.  The library never allocates or
 *    frees device memory the caller sees: the caller passes a workspace sized
 *    by the matching *_workspace_bytes() query.
 *  - Bitboards: Reversi bit = 8*row+col for every board size (the rule entry
 *    points -- bz_reversi_legal / _apply / _game_over / _step_batch_sized --
 *    take size 1..8, every size of the reference's generic constructor,
 *    reversi_board.py:4-14, whose cells fit 64 bits; the engine's games and the
 *    arena are 4, 6 and 8); Tic-tac-toe bit = 3*row+col.  "own" = stones of the side to move,
 *    "opp" = the other side (the side-to-move canonical form of
 *    src/tic_tac_toe/SL/generate_training_games.py:17-18).
 *  - Action index = size*row+col as in the reference's CSV flattening
 *    (generate_training_games.py:42-43); on 8x8 that equals the bit index.
 *    Action 64 = "pass" exists only inside the search tree.
 */
#ifndef BZ_ABI_H
#define BZ_ABI_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BZ_ABI_VERSION 7  /* grown since by additions only: the symmetric forwards, the counted forwards + adaptive shape */

enum { BZ_OK = 0, BZ_EINVAL = 1, BZ_EILLEGAL_MOVE = 2, BZ_EHIP = 3, BZ_ENOMEM = 4, BZ_ENOGPU = 5,
       BZ_ESTATE = 6 };
/* REVERSI = 8x8 (the benchmark game); REVERSI6 / REVERSI4 = the reference's 6x6 and 4x4 demo boards (same
 * bit = 8*row+col, same 65 actions; the conv net serves them through the top-left corner of its 8x8 planes) */
enum { BZ_GAME_TTT = 0, BZ_GAME_REVERSI = 1, BZ_GAME_REVERSI6 = 2, BZ_GAME_REVERSI4 = 3 };
/* leaf evaluators: uniform priors + v=0 (BASELINE cfg 2), synthetic hash (P,v)
 * (tree-kernel parity runs), the conv net in exact-fp32 parity mode, the conv
 * net on bf16 MFMA (the product path), or caller-filled logits/value. */
enum { BZ_EVAL_UNIFORM = 0, BZ_EVAL_HASH = 1, BZ_EVAL_NET_F32 = 2, BZ_EVAL_NET_BF16 = 3,
       BZ_EVAL_EXTERNAL = 4, BZ_EVAL_NET_FP8 = 5,
       /* the reference's tic-tac-toe policy MLP (bz_mlp below, set by bz_engine_set_mlp), BZ_GAME_TTT only:
        * the f32 parity forward or the bf16 MFMA forward.  The reference's net has no value head: value = 0 for
        * every evaluated leaf; a PV handle (bz_mlp_create_pv) gives its own value.  Terminal leaves keep the
        * rules' value either way. */
       BZ_EVAL_MLP_F32 = 6, BZ_EVAL_MLP_BF16 = 7 };
#define BZ_PASS_ACTION 64

int32_t bz_abi_version(void);
const char* bz_last_error(void);
/* the -D flags this library was compiled with ("product" for the shipped build; diagnostic
 * variants carry BZ_EXPERIMENT and are refused by the Python binding unless asked for) */
const char* bz_build_info(void);
/* number of visible HIP devices (0 on a CPU-only host); never fails */
int32_t bz_device_count(void);

/* ------------------------------------------------------------------------ */
/* Scalar rules (host side of the same __host__ __device__ rule functions    */
/* the kernels use).  Back the API-compatible single-board classes.          */
/* ------------------------------------------------------------------------ */
/* ReversiBoard.generate_possible_moves / is_valid_move
 *   src/reversi/game_logic/reversi_board.py:25-41, 87-88.  size 1..8.  Cells that hold neither
 *   side's stones but are not empty (the reference stores any `player` value and treats every
 *   non-zero cell as occupied, :26) are walls: leave them out of own/opp and clear them from
 *   *legal (rays stop at any cell that is not the opponent's, so nothing else changes). */
int32_t bz_reversi_legal(uint64_t own, uint64_t opp, int32_t size, uint64_t* legal);
/* ReversiBoard.make_move  reversi_board.py:43-59.  BZ_EILLEGAL_MOVE where the
 * reference raises ValueError("Invalid move").  Outputs are NOT swapped:
 * own_after = mover's stones after the move. */
int32_t bz_reversi_apply(uint64_t own, uint64_t opp, int32_t size, int32_t row, int32_t col,
                         uint64_t* own_after, uint64_t* opp_after, uint64_t* flips);
/* ReversiBoard.is_game_over  reversi_board.py:61-65 */
int32_t bz_reversi_game_over(uint64_t a, uint64_t b, int32_t size, int32_t* over);
/* ReversiBoard.get_score  reversi_board.py:67-85 (x = +1 stones, o = -1 stones) */
int32_t bz_reversi_score(uint64_t x, uint64_t o, int32_t* winner, int32_t* n_x, int32_t* n_o);
/* TicTacToeBoard.generate_possible_moves  src/tic_tac_toe/tic_tac_toe_board.py:42-43 */
int32_t bz_ttt_legal(uint32_t x, uint32_t o, uint32_t* legal);
/* TicTacToeBoard.make_move  tic_tac_toe_board.py:20-29 */
int32_t bz_ttt_apply(uint32_t own, uint32_t opp, int32_t row, int32_t col, uint32_t* own_after);
/* TicTacToeBoard.is_game_over  tic_tac_toe_board.py:31-40 (+1 tested before -1);
 * *winner is 1/-1/0 and meaningful only when *over != 0 */
int32_t bz_ttt_game_over(uint32_t x, uint32_t o, int32_t* over, int32_t* winner);

/* ------------------------------------------------------------------------ */
/* Batched board-env step (device).  One game per lane.                      */
/* Replaces one iteration of the turn loop in                                */
/*   ReversiTerminal.play  reversi_terminal.py:19-35                         */
/*   TicTacToeHeadless.play  src/tic_tac_toe/tic_tac_toe.py:16-27            */
/* for n games at once.                                                      */
/* ------------------------------------------------------------------------ */
/* status codes written by the step kernels */
enum { BZ_ST_RUNNING = 0, BZ_ST_TERMINAL = 1, BZ_ST_ILLEGAL = 2, BZ_ST_MUST_PASS = 3 };
/* in : own/opp of the mover, action[n] (0..63, or 64 = pass)
 * out: position seen by the NEXT mover (own_next = next mover's stones),
 *      legal_next = next mover's legal mask, status (above; on ILLEGAL the
 *      outputs repeat the inputs), winner = +1/-1/0 for the player who just
 *      moved (valid when TERMINAL).  BZ_ST_MUST_PASS: game not over but the
 *      next mover has no move (the driver flips the side, reversi_terminal.py:32). */
int32_t bz_reversi_step_batch(const uint64_t* own, const uint64_t* opp, const uint8_t* action, int64_t n,
                              uint64_t* own_next, uint64_t* opp_next, uint64_t* legal_next,
                              uint8_t* status, int8_t* winner, void* stream);
/* the same for the reference's smaller boards (size 1..8; bit = 8*row+col; actions are bit
 * indices, 64 = pass) */
int32_t bz_reversi_step_batch_sized(const uint64_t* own, const uint64_t* opp, const uint8_t* action, int64_t n,
                                    int32_t size, uint64_t* own_next, uint64_t* opp_next, uint64_t* legal_next,
                                    uint8_t* status, int8_t* winner, void* stream);
int32_t bz_reversi_legal_batch(const uint64_t* own, const uint64_t* opp, int64_t n, uint64_t* legal,
                               void* stream);
/* ReversiBoard.get_score  reversi_board.py:67-85 for n boards: x = +1 stones, o = -1 stones;
 * winner[n] = +1/-1/0, counts[n][2] = (n_x, n_o) */
int32_t bz_reversi_score_batch(const uint64_t* x, const uint64_t* o, int64_t n, int8_t* winner,
                               uint8_t* counts, void* stream);
/* Tic-tac-toe: to_move[n] = absolute colour (+1/-1) of the mover; winner is the
 * ABSOLUTE colour (+1/-1/0) exactly as TicTacToeBoard.is_game_over returns it. */
int32_t bz_ttt_step_batch(const uint16_t* own, const uint16_t* opp, const uint8_t* action,
                          const int8_t* to_move, int64_t n, uint16_t* own_next, uint16_t* opp_next,
                          uint16_t* legal_next, uint8_t* status, int8_t* winner, void* stream);

/* 8-fold symmetry augmentation of (s, pi) rows on the device -- the transforms of
 * TicTacToeDataset.expand_with_transforms, src/tic_tac_toe/SL/train.py:27-36, in the
 * reference's order (id, flip rows, flip cols, rot90 x1/x2/x3, transpose, flip-rows-then-
 * transpose; the last equals rot90 x3 under torch semantics, as in the reference).
 * Row 8*i+t of the outputs = transform t of input row i; pi is permuted with the board
 * (entries beyond size*size -- Reversi's pass -- stay).  key8 (optional, may be null) gets a
 * 64-bit content key of each output row for the dedupe of train.py:45-50.  n == 0 is a no-op
 * whatever the pointers are (an empty tensor has a null data pointer). */
int32_t bz_augment_d4_batch(const uint64_t* own, const uint64_t* opp, const float* pi, int64_t n, int32_t size,
                            int32_t na, uint64_t* own8, uint64_t* opp8, float* pi8, uint64_t* key8, void* stream);

/* ------------------------------------------------------------------------ */
/* The reference's minimax players (the arena's yard-stick, SURVEY.md 8(f)   */
/* row 3), one game per lane, and as scalar host entry points.               */
/* ------------------------------------------------------------------------ */
/* OptimalPlayer.minimax  src/reversi/players/reversi_players.py:41-69 with evaluate_board :71-77:
 * depth-limited (any max_depth >= 0 for the scalar entry point; 0 <= max_depth <= 8 for the batched kernel, whose
 * stack lives in a lane's registers / scratch), stone difference for the player, moves in
 * generate_possible_moves order, first strictly better score wins, no pass rule inside the
 * search (a side without a move in an unfinished game scores -inf / +inf: the reference's
 * behaviour).  self = the player's stones, other = the opponent's; the player is to move.
 * *move = bit index 8*row+col, or -1 where the reference's best_move is None (get_move then
 * draws random.choice, :38-39 -- left to the caller); *score = the root value (+-1000 = +-inf). */
int32_t bz_reversi_minimax(uint64_t self, uint64_t other, int32_t size, int32_t max_depth, int32_t* move,
                           int32_t* score);
/* OptimalPlayer.minimax  src/tic_tac_toe/players.py:41-70 (full depth; +1/0/-1 for the player).
 * symbol = the player's colour (+1 = X), needed only for is_game_over's X-before-O test order.
 * *move = 3*row+col, -1 = None (finished board), -2 = empty board (the reference plays a random
 * opening move there, :35-36 -- left to the caller). */
int32_t bz_ttt_minimax(uint32_t self, uint32_t other, int32_t symbol, int32_t* move, int32_t* score);
/* batched: device arrays [n]; active (optional, may be null): 0 = skip the game (move -1) */
int32_t bz_reversi_minimax_batch(const uint64_t* self, const uint64_t* other, const uint8_t* active, int64_t n,
                                 int32_t size, int32_t max_depth, int8_t* move, int16_t* score, void* stream);
int32_t bz_ttt_minimax_batch(const uint16_t* self, const uint16_t* other, const int8_t* symbol,
                             const uint8_t* active, int64_t n, int8_t* move, int16_t* score, void* stream);

/* ------------------------------------------------------------------------ */
/* Policy/value net (build-authored architecture, SURVEY.md 8(d) "net";      */
/* the calling convention generalises AIPlayer.get_move players.py:84-98:    */
/* side-to-move canonical input, logits out, legality masked by the caller)  */
/* ------------------------------------------------------------------------ */
typedef struct bz_net bz_net;
/* flat fp32 parameter vector, torch layouts, in this order:
 *  stem.w[C][2][3][3] stem.b[C] { c1.w[C][C][3][3] c1.b[C] c2.w[C][C][3][3] c2.b[C] } x NB
 *  pol.w[2][C] pol.b[2] polfc.w[65][128] polfc.b[65]
 *  val.w[1][C] val.b[1] v1.w[VH][64] v1.b[VH] v2.w[1][VH] v2.b[1] */
int64_t bz_net_param_count(int32_t C, int32_t NB, int32_t VH);
int64_t bz_net_workspace_bytes(int32_t C, int32_t NB, int32_t VH, int32_t max_batch);
/* params_host: host pointer.  Repacks + uploads weights into the workspace
 * (synchronises the stream once). */
int32_t bz_net_create(int32_t C, int32_t NB, int32_t VH, int32_t max_batch, const float* params_host,
                      void* workspace, int64_t workspace_bytes, void* stream, bz_net** out);
int32_t bz_net_destroy(bz_net* net);
/* replace the weights of an existing net (same shape) -- after a training step */
int32_t bz_net_update(bz_net* net, const float* params_host, void* stream);
/* own/opp: device u64[n]; logits: device f32[n][65]; value: device f32[n].
 * _f32: exact parity mode (k-ordered fmaf chains == oracle bit for bit).
 * _bf16: MFMA path (bf16 activations/weights, fp32 accumulate); C = 64, 128 or 256
 *        (C = 32 nets run on the _f32 path only).
 * Every ReLU of all three paths is torch's, IEEE maximum(y, +0): a NaN of either sign passes (a NaN
 * weight stays a NaN through the bf16 / e4m3 packing), -0 becomes +0.  A net with a NaN or infinite
 * parameter thus gives a non-finite logit or value wherever torch's fp32 PolicyValueNet does (except
 * through the products with the board's zero padding, which the kernels skip), and the engine's
 * ERR_EVAL_NONFINITE guard fires on it. */
int32_t bz_net_forward_f32(bz_net* net, const uint64_t* own, const uint64_t* opp, int32_t n,
                           float* logits, float* value, void* stream);
int32_t bz_net_forward_bf16(bz_net* net, const uint64_t* own, const uint64_t* opp, int32_t n,
                            float* logits, float* value, void* stream);
/* _fp8: e4m3 weights (per-output-channel power-of-two scale) and activations (x16) on the
 * MX-scaled 32x32x64 MFMA (BASELINE config 5); pass parameters fake-quantised by
 * betazero_amd/quant.py.  Needs C == 128.  The activation store saturates at 448 (+inf included);
 * a NaN is stored as the e4m3fn NaN code and carries into the next layer. */
int32_t bz_net_forward_fp8(bz_net* net, const uint64_t* own, const uint64_t* opp, int32_t n,
                           float* logits, float* value, void* stream);

/* ---- device-side row counts and the adaptive tower shape (an addition to ABI 7) ----
 * _counted: the forward over the first *n_dev rows (device u32) of buffers of max_n <= max_batch rows -- the call the
 * engine makes with its packed-leaf count.  Rows >= *n_dev are never written; a count of 0 touches no memory.  A count
 * above max_n is clamped to max_n on the device (rows, shape and tally are those of max_n rows): no count reaches past
 * the buffers.  Counts of 2^31 and above are outside the contract: they read as negative and run nothing.  Every row is
 * bit for bit what the host-count forward gives (tests/test_gpu_net_counted.py).
 * At C == 128, bf16 and max_n > 256 the tower's workgroup shape follows the count: the latency shape (one position per
 * workgroup) up to the threshold, the throughput shape above it; both are launched and the one the count rules out exits
 * at once.  Every row is bit for bit what either shape gives (they agree by construction of the accumulation order).
 * bz_net_set_adaptive_shape: 1 = on (the default), 0 = off (the throughput shape whatever the count: what every
 *   device-count launch did before the shape adapted), 2 = the latency shape whatever the count (measurement: tools/bench_tower_shapes.py).  Takes effect
 *   for the launches issued after it.  Host-count forwards never adapt.
 * bz_net_shape_tally: counts[3] = such launches that did work since the last call, by shape {latency, middle (no such
 *   tier is built: always 0), throughput}, counted on the device by the launch itself (a count of 0 runs no shape);
 *   reads and clears behind the work queued on `stream` and synchronises it. */
int32_t bz_net_forward_counted(bz_net* net, int32_t kind, const uint64_t* own, const uint64_t* opp, int32_t max_n,
                               const uint32_t* n_dev, float* logits, float* value, void* stream);
int32_t bz_net_set_adaptive_shape(bz_net* net, int32_t mode);
int32_t bz_net_shape_tally(bz_net* net, int64_t* counts /* [3] */, void* stream);
/* bz_net_set_tile_map (an addition to ABI 7): which kernel runs the throughput shape of the plain bf16 forward
 *   at C == 128, with a host count or a device count (the adaptive pair's high window included): 1 = k_edge_bf16 on the
 *   edge-aware cell tiling (csrc/bz_tile_map.h; the default), 0 = k_tower_bf16 on board-row tiles.  Every row is bit for bit
 *   the same under both; both count in the throughput slot of bz_net_shape_tally.  The symmetric forward, the latency
 *   shape, the other widths and fp8 do not depend on it.  Takes effect for the launches issued after it. */
int32_t bz_net_set_tile_map(bz_net* net, int32_t map);

/* ---- the forward under a board symmetry ----
 * Eight elements s = 0..7 on the size x size corner of the 8x8 planes: 0..6 are bz_augment_d4_batch's transforms 0..6
 * (id, flip rows, flip columns, rot90 x1, x2, x3, transpose), 7 is the anti-transpose out[r][c] = x[n-1-c][n-1-r] (which
 * the reference's augmentation list lacks: its entry 7 repeats entry 5).  T_s moves a stone on cell j to tau_s(j); cells
 * outside the corner and the pass action stay, so tau_s permutes 0..63 and fixes 64.
 * bz_sym_index: the symmetry a position is evaluated under for a seed -- a hash of (seed, own, opp), so the evaluator stays
 *   a function of the position alone (evaluation cache, carry-over and bit-for-bit replays keep their guarantees):
 *     h = seed ^ (own * 0x9E3779B97F4A7C15); h = (h ^ (h >> 29)) * 0xBF58476D1CE4E5B9; h ^= opp * 0xC2B2AE3D27D4EB4F;
 *     h = (h ^ (h >> 32)) * 0x94D049BB133111EB; s = (h ^ (h >> 31)) >> 61            (64-bit wrapping arithmetic)
 * bz_sym_board: *out = T_s(b), size 1..8.  bz_sym_action_map: map[j] = tau_s(j), j = 0..64.  Host only, per item. */
uint32_t bz_sym_index(uint64_t seed, uint64_t own, uint64_t opp);
int32_t bz_sym_board(uint64_t b, int32_t size, int32_t s, uint64_t* out);
int32_t bz_sym_action_map(int32_t size, int32_t s, uint8_t* map /* [65] */);
enum { BZ_SYM_FIXED = 0, BZ_SYM_HASHED = 1, BZ_SYM_MEAN = 2 };
/* kind: 0 = f32, 1 = bf16, 2 = fp8 (the shapes of the plain forwards); size 8, 6 or 4.  Per row, with L', v' what the plain
 * forward gives on (T_s own, T_s opp): logits[j] = L'[tau_s(j)] (j < 64), logits[64] = L'[64], value = v'.  The transform
 * and the permuted store are fused into the net kernels (separate instantiations: the plain forwards are untouched).
 *   BZ_SYM_FIXED  (arg = s): every row under T_s.
 *   BZ_SYM_HASHED (arg = seed): row i under s_i = bz_sym_index(seed, own_i, opp_i), computed in the kernel.
 *   BZ_SYM_MEAN: the eight FIXED forwards into `scratch` (device memory, 256-byte aligned, bz_net_sym_scratch_bytes(n)
 *     bytes), then ((..(x_0 + x_1) + ..) + x_7) * 0.125f in fp32 per logit and per value.  arg is ignored.
 * scratch may be null for FIXED and HASHED. */
int64_t bz_net_sym_scratch_bytes(int64_t n);
int32_t bz_net_forward_sym(bz_net* net, int32_t kind, const uint64_t* own, const uint64_t* opp, int32_t n, int32_t size,
                           int32_t mode, uint64_t arg, void* scratch, int64_t scratch_bytes, float* logits, float* value,
                           void* stream);
/* the same over the first *n_dev rows (see bz_net_forward_counted); FIXED and HASHED only */
int32_t bz_net_forward_sym_counted(bz_net* net, int32_t kind, const uint64_t* own, const uint64_t* opp, int32_t max_n,
                                   const uint32_t* n_dev, int32_t size, int32_t mode, uint64_t arg, float* logits,
                                   float* value, void* stream);

/* ------------------------------------------------------------------------ */
/* The reference's tic-tac-toe policy MLP, TicTacToeNet                       */
/*   src/tic_tac_toe/SL/neural_networks.py: Linear(9,H)-ReLU-Linear(H,H)-     */
/*   ReLU-Linear(H,H)-ReLU-Linear(H,9), logits only; H = 256 shipped.         */
/* Played by AIPlayer.get_move (players.py:76-104), trained by SL/train.py.   */
/* ------------------------------------------------------------------------ */
typedef struct bz_mlp bz_mlp;
/* H: a multiple of 32 in 32..512.  Flat fp32 parameter vector in torch's order:
 *  fc1.w[H][9] fc1.b[H] fc2.w[H][H] fc2.b[H] fc3.w[H][H] fc3.b[H] fc4.w[9][H] fc4.b[9]
 * Both return -1 (bz_last_error) for an H out of range / max_batch < 1. */
int64_t bz_mlp_param_count(int32_t H);
int64_t bz_mlp_workspace_bytes(int32_t H, int32_t max_batch);
/* params_host: host pointer.  Repacks + uploads the weights into the workspace (synchronises the stream once). */
int32_t bz_mlp_create(int32_t H, int32_t max_batch, const float* params_host, void* workspace, int64_t workspace_bytes,
                      void* stream, bz_mlp** out);
int32_t bz_mlp_destroy(bz_mlp* mlp);
/* replace the weights (same H); drains the device first, like bz_net_update */
int32_t bz_mlp_update(bz_mlp* mlp, const float* params_host, void* stream);
/* own/opp: device u64[n], side to move canonical, cell i = bit i (row-major), input x_i = own_i - opp_i;
 * _states: device f32 x[n][9] as the reference feeds it (symbol * board).  logits: device f32[n][9].  n <= max_batch.
 * _f32: fp32 parity mode, one fmaf chain per output over k = 0, 1, ..., K-1 from 0, then + bias -- a row's logits do
 *       not depend on the batch it is in or on the run.
 * _bf16: bf16 weights and activations, fp32 accumulation, on v_mfma_f32_16x16x32_bf16. */
int32_t bz_mlp_forward_f32(bz_mlp* mlp, const uint64_t* own, const uint64_t* opp, int32_t n, float* logits, void* stream);
int32_t bz_mlp_forward_bf16(bz_mlp* mlp, const uint64_t* own, const uint64_t* opp, int32_t n, float* logits, void* stream);
int32_t bz_mlp_forward_states_f32(bz_mlp* mlp, const float* x, int32_t n, float* logits, void* stream);
int32_t bz_mlp_forward_states_bf16(bz_mlp* mlp, const float* x, int32_t n, float* logits, void* stream);
/* One supervised step of SL/train.py: loss = sum_r w_r CE(logits_r, target_r) / sum_r w_r (w_r = 1 when row_w is null:
 * torch's CrossEntropyLoss mean), then torch.optim.Adam (no weight decay) with the bias corrections of step `step`.
 * Two launches.  Everything is a caller-owned DEVICE buffer except `adam` (host):
 *   params/m/v: fp32 [bz_mlp_param_count] (torch order; params must hold the weights the mlp was created / updated
 *     with -- the step keeps both in step); grad (optional): the batch gradient;
 *   x f32 [n][9], target i32 [n] (0..8 = the reference's action.argmax(1)), row_w f32 [n] (optional; 0 = row ignored,
 *     so a short last batch needs no second shape); loss f32 [1] (optional); logits f32 [n][9] (optional, forward output);
 *   ws: bz_mlp_train_workspace_bytes(H, n) bytes, 256-byte aligned.
 * err (u32, sticky: the step ORs into it, the caller clears it): 1 = a target outside 0..8 on a row of non-zero weight,
 * 2 = a non-finite loss, 4 = the row weights sum to <= 0.  While *err != 0 the step changes no parameter or moment.
 * The betas are float32; Adam is torch's formula at those betas: 1 - beta is taken in fp32 from the float beta (exact),
 * the bias corrections 1 - beta^step in double from it.  (torch.optim.Adam takes 1 - beta in double from the Python
 * float: at beta2 = 0.999 its v differs from this one by 1.3e-5 relative; the parameters do not measurably.) */
typedef struct bz_mlp_adam {
    float lr, beta1, beta2, eps;  /* SL/train.py: 1e-4, 0.9, 0.999, 1e-8 */
    int32_t step;                 /* 1 for the first step */
} bz_mlp_adam;
int64_t bz_mlp_train_workspace_bytes(int32_t H, int32_t max_batch);
int32_t bz_mlp_train_step(bz_mlp* mlp, float* params, float* m, float* v, float* grad, const float* x,
                          const int32_t* target, const float* row_w, int32_t n, const bz_mlp_adam* adam,
                          void* ws, int64_t ws_bytes, float* loss, float* logits, uint32_t* err, void* stream);

/* The MLP with a value head, TicTacToePVNet (betazero_amd/mlp.py): fc1..fc3 are the reference's, fc4 = Linear(H, 10); rows
 * 0..8 are the policy logits, row 9 is the value pre-activation u and v = tanh(u).  Flat order as above with fc4.w[10][H]
 * fc4.b[10]: 2 H^2 + 22 H + 10 floats.  A PV handle is a bz_mlp: destroy, update (its own parameter count), the engine
 * (bz_engine_set_mlp: BZ_EVAL_MLP_* then put v on the evaluated leaves) and the four forwards above (logits alone) take it.
 * _pv_ forwards: value f32 [n] as well; BZ_EINVAL on a handle of bz_mlp_create.
 *   _f32: unit 9 runs through the same fmaf chain as the logits, then tanhf_spec (the conv net's value head's);
 *   _bf16: row 9 of fc4's one MFMA tile, + bias, tanhf_spec -- no instruction more than the policy-only forward's tile. */
int64_t bz_mlp_pv_param_count(int32_t H);
int64_t bz_mlp_pv_workspace_bytes(int32_t H, int32_t max_batch);
int32_t bz_mlp_create_pv(int32_t H, int32_t max_batch, const float* params_host, void* workspace, int64_t workspace_bytes,
                         void* stream, bz_mlp** out);
int32_t bz_mlp_has_value(const bz_mlp* mlp);   /* 1 = a handle of bz_mlp_create_pv */
int32_t bz_mlp_forward_pv_f32(bz_mlp* mlp, const uint64_t* own, const uint64_t* opp, int32_t n, float* logits, float* value,
                              void* stream);
int32_t bz_mlp_forward_pv_bf16(bz_mlp* mlp, const uint64_t* own, const uint64_t* opp, int32_t n, float* logits, float* value,
                               void* stream);
int32_t bz_mlp_forward_pv_states_f32(bz_mlp* mlp, const float* x, int32_t n, float* logits, float* value, void* stream);
int32_t bz_mlp_forward_pv_states_bf16(bz_mlp* mlp, const float* x, int32_t n, float* logits, float* value, void* stream);
/* One AlphaZero step on a PV handle: loss = sum_r (w_r / sum w) [ sum_o pi_o (lse(z) - z_o) + value_weight (v - vt)^2 ], the
 * logits unmasked; then Adam exactly as bz_mlp_train_step.  Two launches.  Buffers as there, with
 *   params/m/v/grad: fp32 [bz_mlp_pv_param_count]; pi f32 [n][9] >= 0 (need not sum to 1: the gradient on logit o is
 *     scale (S p_o - pi_o), S = sum_o pi_o in ascending o); vt f32 [n] in [-1, 1]; value f32 [n] (optional, forward output);
 *   gradient on u: scale value_weight 2 (v - vt) (1 - v^2);  ws: bz_mlp_train_pv_workspace_bytes(H, n) bytes.
 * err: 1 = on a row of non-zero weight a negative or non-finite pi entry, sum pi <= 0, or vt non-finite / outside [-1, 1];
 * 2 = a non-finite loss; 4 = the row weights sum to <= 0.  While *err != 0 the step changes no parameter or moment. */
int64_t bz_mlp_train_pv_workspace_bytes(int32_t H, int32_t max_batch);
int32_t bz_mlp_train_step_pv(bz_mlp* mlp, float* params, float* m, float* v, float* grad, const float* x, const float* pi,
                             const float* vt, const float* row_w, int32_t n, float value_weight, const bz_mlp_adam* adam,
                             void* ws, int64_t ws_bytes, float* loss, float* logits, float* value, uint32_t* err, void* stream);

/* ------------------------------------------------------------------------ */
/* Batched MCTS self-play engine.  The plug-in point it fills is             */
/*   Player.get_move(board)  src/tic_tac_toe/players.py:6-9,                 */
/*   ReversiPlayer.get_move  src/reversi/players/reversi_players.py:5-8      */
/* (one search per call) and, batched, the game loops cited above plus the   */
/* example extraction of generate_training_games.py:12-38.                   */
/* ------------------------------------------------------------------------ */
typedef struct bz_engine bz_engine;
typedef struct bz_engine_cfg {
    int32_t game;        /* BZ_GAME_* */
    int32_t n_games;     /* concurrent game slots B on this GPU */
    int32_t sims;        /* simulations per move */
    int32_t eval_kind;   /* BZ_EVAL_* */
    float c_puct;        /* 1.5 in every BASELINE config */
    int32_t temp_moves;  /* moves_made < temp_moves -> sample ~ N (tau=1), else argmax N */
    int32_t openings;    /* Reversi: first 2 plies from the 12 fixed openings (game_id % 12) */
    int32_t rounds;      /* example-buffer depth: slot s plays games s, s+stride, ... (>=1) */
    int32_t t_max;       /* example rows per game (64 Reversi, 9 TTT) */
    int32_t stagger;     /* bench only: slot g starts its round-0 game pre-advanced by (g % stagger)
                          * pseudo-random plies so that completions are spread evenly (0 = off) */
    uint64_t seed;
    uint64_t game_id_base;   /* global id of slot 0, round 0 (= rank * n_games) */
    uint64_t game_id_stride; /* id distance between rounds (= world_size * n_games) */
    /* opt-in search features (all zero = the BASELINE configurations) */
    uint32_t flags;          /* BZ_ENGINE_* bits */
    float dirichlet_alpha;   /* 0 < alpha <= 1 when dirichlet_eps > 0 */
    float dirichlet_eps;     /* > 0: root priors P' = (1 - eps) P + eps Dirichlet(alpha), a fresh draw per
                              * search keyed by (seed, game id, moves made) -- DESIGN.md 3.9 */
    int32_t ttt_lanes;       /* tic-tac-toe fused search (synthetic evaluators, sims <= 120): lanes that serve one game --
                              * 0 = default (4), 1 / 2 / 4 / 8 = as given, -1 = the generic
                              * any-game fused kernel.  Results are identical for every setting. */
} bz_engine_cfg;
/* The tree's edge record packs (visits 14 bits | action | the child's edge count, terminal flag and value) and
 * (child id 13 bits | the child's first edge 19 bits) into two words, so a game's tree holds at most 8191 nodes:
 * sims <= 8189, or <= 2045 with BZ_ENGINE_REUSE_SUBTREE (the arena then holds 4 x (sims + 2) nodes).  Larger
 * values are refused with BZ_EINVAL. */
#define BZ_ENGINE_MAX_SIMS 8189
#define BZ_ENGINE_MAX_SIMS_REUSE 2045
/* keep the chosen child's subtree as the next search's tree; searches then go through the
 * step kernels for every evaluator */
#define BZ_ENGINE_REUSE_SUBTREE 1u
/* Evaluation cache (conv net evaluators; ignored with the synthetic / external / MLP evaluators, with BZ_ENGINE_REUSE_SUBTREE
 * and with more than one leaf per step, BZ_ENGINE_LEAVES_*):
 * a leaf whose position was already evaluated earlier in the SAME search -- reached by another move order -- takes that
 * node's priors and value instead of an evaluator row.  The evaluator is a function of the position alone
 * (players.py:84-98: canonical planes in, logits out), so every result (visit counts, W, P, pi, moves) is bit for
 * bit what it is without the cache -- the tree is the same tree, only the repeated forward is not run.  The work counters
 * say how often: counters[8] = repeats served from the cache, counters[7] = rows the evaluator computed; their sum is
 * what counters[7] reads without the cache.  A table hit is confirmed against the stored node's position before use. */
#define BZ_ENGINE_EVAL_CACHE 2u
/* ... and across CONSECUTIVE searches of a slot (with BZ_ENGINE_EVAL_CACHE): the previous search's tree stays intact in a
 * second arena while the new one grows (the arenas alternate), and a leaf whose position that tree evaluated takes the
 * evaluation from there.  After a move the new root is a child of the old one, and a fresh search from it re-creates that
 * child's old subtree node for node (deterministic PUCT on the same evaluations), so about the played move's share of the
 * previous search's visits -- a quarter at cfg 3 -- never reaches the net again.  The new tree is still built from scratch
 * (this is NOT subtree reuse: no statistic is kept, DESIGN.md 3.10 stays an option of its own): results are bit for bit
 * those without any cache.  counters[9] = the part of counters[8] that came from the previous search.  Nothing is carried
 * over a change of weights: a search that follows bz_net_update / bz_engine_set_net starts with the in-search cache only. */
#define BZ_ENGINE_EVAL_CACHE_CARRY 4u
/* Leaf-parallel search: bits 8..12 of flags hold K - 1, K = leaves per step per game (1..32; 0 in the
 * field = K = 1 = the one-walk-per-step engine, unchanged).  With K > 1 every tree step runs K' = min(K, sims - done) PUCT
 * walks per game, each leaving a virtual loss (N += 1, W -= 1) on its path for the next, and the evaluator takes up to
 * K x n_games rows per launch.  A walk that reaches a node an earlier walk of the same step created (not expanded yet)
 * stops there and backs up that node's value: counters[10] (n_collisions).  The evaluation cache is ignored with K > 1;
 * the synthetic evaluators then run through the step kernels.  Bits above 12 are refused (BZ_EINVAL).
 * Workspace with K > 1: the select paths [B][K][MAXD], a 32-byte record per leaf [B][K] (node, header, legal mask, evaluator
 * row, depth, kind) and K x B leaf / evaluator rows (bz_engine_layout). */
#define BZ_ENGINE_LEAVES_SHIFT 8
#define BZ_ENGINE_LEAVES_MASK (31u << BZ_ENGINE_LEAVES_SHIFT)

/* offsets (bytes, from the workspace base) of the caller-visible arrays */
typedef struct bz_engine_layout {
    int64_t ex_own, ex_opp;   /* u64 [rounds][B][t_max]  side-to-move canonical s */
    int64_t ex_pi;            /* f32 [rounds][B][t_max][NA]  pi = N/sum N            */
    int64_t ex_z;             /* i8  [rounds][B][t_max]  outcome for the mover       */
    int64_t ex_mover, ex_act; /* i8 / u8 [rounds][B][t_max]                          */
    int64_t ex_len;           /* i32 [rounds][B]  rows valid (-1 = game not finished) */
    int64_t ex_winner;        /* i8  [rounds][B]  absolute winner                    */
    int64_t root_N, root_W, root_P; /* u32/f32/f32 [B][NA] filled by bz_engine_root_stats */
    /* leaf rows: K x B with K leaves per step (BZ_ENGINE_LEAVES_*), row g*K + j = walk j of game g (K = 1: row g).
     * Net / MLP evaluators read the leaves packed by slot instead; logits / value then hold the packed rows. */
    int64_t leaf_own, leaf_opp;     /* u64 [K*B]   positions awaiting evaluation     */
    int64_t leaf_kind;              /* u8  [K*B]   1 = needs (logits,value)           */
    int64_t logits, value;          /* f32 [K*B][NA], f32 [K*B]  evaluator outputs    */
    int64_t g_own, g_opp;           /* u64 [B] current positions                      */
    int64_t g_to_move, g_state;     /* i8 / u8 [B]  (state: 0 active, 1 finished)     */
    int64_t counters;               /* u64 [24] work counters: 0..10 used */
    int32_t na, t_max;
    /* The example arrays ex_own .. ex_winner are consecutive in the workspace and are followed by
     * a 256-byte header (ex_meta: u64 magic, game_id_base, game_id_stride, B, rounds, t_max, NA,
     * game, then the 8 array offsets relative to ex_begin).  [ex_begin, ex_begin + ex_bytes) is the
     * ONE contiguous, self-describing byte range that the iteration-end all-gather ships. */
    int64_t ex_begin, ex_bytes, ex_meta;
} bz_engine_layout;

int64_t bz_engine_workspace_bytes(const bz_engine_cfg* cfg);
int32_t bz_engine_create(const bz_engine_cfg* cfg, void* workspace, int64_t workspace_bytes,
                         bz_engine** out);
int32_t bz_engine_destroy(bz_engine* e);
int32_t bz_engine_get_layout(const bz_engine* e, bz_engine_layout* out);
int32_t bz_engine_set_net(bz_engine* e, bz_net* net);
/* the MLP of BZ_EVAL_MLP_F32 / BZ_EVAL_MLP_BF16 (engines of BZ_GAME_TTT; those eval kinds with any other game are
 * refused with BZ_EINVAL by bz_engine_workspace_bytes / bz_engine_create).  Its max_batch must be >= n_games; with K > 1
 * leaves per step bz_engine_set_mlp (and bz_engine_set_net for a net) refuse a max_batch below K x n_games. */
int32_t bz_engine_set_mlp(bz_engine* e, bz_mlp* mlp);
/* test hook: set the count of searches begun so far (0 .. 2^19 - 3) -- the evaluation cache stamps its entries with it, cycling
 * through 1 .. 2^19 - 2; a test starts just below the wrap with this.  Nothing is carried over the jump. */
int32_t bz_engine_debug_set_search_seq(bz_engine* e, uint32_t seq);
/* Hashed evaluation symmetry, opt-in per engine, between searches.  on != 0: bz_engine_evaluate evaluates
 * every packed leaf (the device-side count path included) by bz_net_forward_sym(.., BZ_SYM_HASHED, seed, ..) with the game's
 * board size, i.e. under the symmetry bz_sym_index(seed, own, opp) of its own position.  The evaluator stays a function of
 * the position alone, so the evaluation cache, its carry-over, subtree reuse, leaves_per_step, Gumbel, the playout cap, forced
 * playouts, surprise, the search value and matches keep every guarantee they give without it.  The setting lives on the
 * engine, not on the bz_net (two pipelines, or the two players of a match, share one net).  on == 0 (the default): the plain
 * forward, the kernels and the bits of an engine that never heard of it.  BZ_EINVAL for on != 0 on tic-tac-toe and on the
 * uniform / hash / external / MLP evaluators.  The cache's rule "nothing is carried over a change of weights" extends to a
 * change of the setting or of the seed. */
int32_t bz_engine_set_eval_symmetry(bz_engine* e, int32_t on, uint64_t seed);
/* start every slot at the game's start position (round 0) */
int32_t bz_engine_reset_games(bz_engine* e, void* stream);
/* load arbitrary root positions (MCTSPlayer.get_move, the arena, tests): device arrays [B];
 * to_move[g] = +1 / -1 (absolute colour of the mover) or 0 = leave slot g idle in this search */
int32_t bz_engine_set_roots(bz_engine* e, const uint64_t* own, const uint64_t* opp,
                            const int8_t* to_move, void* stream);
/* one full search (root expansion + cfg.sims simulations) for every active slot */
int32_t bz_engine_search(bz_engine* e, void* stream);
/* the search, step by step (BZ_EVAL_EXTERNAL callers fill logits/value between) */
int32_t bz_engine_root_begin(bz_engine* e, void* stream);   /* roots -> leaf buffers       */
/* sim_index = simulations already completed in this search (0, 1, 2, ...); with K leaves per step 0, K, 2K, ...:
 * the call starts the next min(K, sims - sim_index) walks of every active slot */
int32_t bz_engine_select(bz_engine* e, uint32_t sim_index, void* stream); /* M2: PUCT walk + env step */
int32_t bz_engine_evaluate(bz_engine* e, void* stream);     /* run cfg.eval_kind on leaves */
int32_t bz_engine_expand_backup(bz_engine* e, void* stream);/* M3 + M4                     */
/* Dirichlet root noise (cfg.dirichlet_eps > 0; a no-op otherwise) on the priors of the expanded roots, and with Gumbel root
 * search on (bz_engine_set_gumbel) the per-search Gumbel preparation of the expanded roots.  Step-API
 * callers run it once per search, after the expand_backup that follows root_begin and before select(0) -- the order
 * bz_engine_search uses. */
int32_t bz_engine_root_noise(bz_engine* e, void* stream);
/* copy root edge statistics into the root_N/W/P arrays, indexed by action */
int32_t bz_engine_root_stats(bz_engine* e, void* stream);
/* M5: pi, move choice, example row, env step, pass rule, terminal handling.
 * restart != 0: a finished slot starts its next game (next round) at once. */
int32_t bz_engine_play(bz_engine* e, int32_t restart, void* stream);
/* ---- The search options and the pairs that do not run together ("The search mode").  Fifteen switches change what a
 * search does or records; three travel in the config (subtree reuse, leaves per step, Dirichlet noise), the others have a
 * setter.  THE list of refused pairs, each in either order (csrc/bz_options.h is its code):
 *   subtree reuse, and leaves_per_step > 1, with each of Gumbel root search, the playout cap, forced playouts, first-play urgency
 *     reduction, the solver (concurrent walks race on proofs) and early stop;
 *   Dirichlet noise with Gumbel root search;
 *   Gumbel root search with the playout cap, forced playouts, first-play urgency reduction, the solver and early stop (sequential
 *     halving is its own schedule);
 *   the solver with forced playouts (both score +inf), first-play urgency reduction and early stop;
 *   early stop with the playout cap, forced playouts, the root store (a shortened tree must not seed a later search) and the
 *     observers surprise, search value, ownership and resignation (their targets and records come from complete searches);
 *   ownership with resignation (a resigned game has no final board).
 * Every other pair runs together.  A setter that would complete a refused pair returns BZ_EINVAL, a *_bytes function -1 and a
 * *_check function BZ_EINVAL for a config that carries one half of it, and bz_last_error names the function, both options and how
 * the other one is switched on.  (The Gumbel interior rule needs Gumbel root search and otherwise combines with what that
 * combines with: a requirement, not a pair.) */
enum {
    BZ_OPT_REUSE_SUBTREE = 0,   /* cfg.flags & BZ_ENGINE_REUSE_SUBTREE */
    BZ_OPT_LEAVES = 1,          /* cfg.flags: BZ_ENGINE_LEAVES_* says more than one leaf per step */
    BZ_OPT_DIRICHLET = 2,       /* cfg.dirichlet_eps > 0 */
    BZ_OPT_GUMBEL = 3,          /* bz_engine_set_gumbel */
    BZ_OPT_GUMBEL_INTERIOR = 4, /* bz_engine_set_gumbel_interior */
    BZ_OPT_PLAYOUT_CAP = 5,     /* bz_engine_set_playout_cap */
    BZ_OPT_FORCED_PLAYOUTS = 6, /* bz_engine_set_forced_playouts */
    BZ_OPT_FPU = 7,             /* bz_engine_set_fpu */
    BZ_OPT_SOLVER = 8,          /* bz_engine_set_solver */
    BZ_OPT_EARLY_STOP = 9,      /* bz_engine_set_early_stop */
    BZ_OPT_ROOT_STORE = 10,     /* bz_engine_set_root_store */
    BZ_OPT_SURPRISE = 11,       /* bz_engine_set_surprise */
    BZ_OPT_SEARCH_VALUE = 12,   /* bz_engine_set_search_value */
    BZ_OPT_OWNERSHIP = 13,      /* bz_engine_set_ownership */
    BZ_OPT_RESIGN = 14,         /* bz_engine_set_resign */
    BZ_OPT_COUNT = 15
};
/* 1 when options a and b (BZ_OPT_*) are a refused pair, 0 when they run together (a == b included); -1 for an id outside
 * 0 .. BZ_OPT_COUNT - 1.  Host only. */
int32_t bz_option_conflict(int32_t a, int32_t b);
/* the phrase the refusals use for option a (static storage), or null for an id outside 0 .. BZ_OPT_COUNT - 1.  Host only. */
const char* bz_option_name(int32_t a);
/* Gumbel root search (Danihelka et al., ICLR 2022), opt-in per engine.  The root's edge of every walk is
 * chosen by Gumbel-top-k sampling plus sequential halving over the max_considered best root actions; every deeper level of
 * the walk stays PUCT.  The move is the considered action that survives the halving, and the example row's pi is the improved
 * policy softmax(log P + sigma(completed Q)).  Gumbel noise is drawn while moves made < cfg.temp_moves and gumbel_scale > 0
 * (tau = 1 visit sampling is not used in this mode).  Refused combinations: the list at BZ_OPT_*.  The evaluation cache works
 * unchanged.  Searches go through the step kernels. */
#define BZ_GUMBEL_MAX_CONSIDERED 64
/* bytes of the caller-owned Gumbel buffer for cfg and max_considered (1..64): the considered-visit table u16
 * [max_considered][sims], every root edge's base value f32 [n_games][MAXCH] and the root's value f32 [n_games], each array
 * 256-byte aligned.  Needs no GPU; -1 (bz_last_error says why) for bad arguments or a refused combination. */
int64_t bz_engine_gumbel_bytes(const bz_engine_cfg* cfg, int32_t max_considered);
/* switch Gumbel root search on (max_considered 1..64; defaults of mctx's gumbel_muzero_policy: 16, gumbel_scale 1.0,
 * maxvisit_init 50.0, value_scale 0.1) or off (max_considered 0), between searches.  buf: device memory of
 * >= bz_engine_gumbel_bytes bytes, 256-byte aligned, owned by the caller and kept alive while the mode is on.  The
 * considered-visit table is filled at once (the call synchronises `stream`). */
int32_t bz_engine_set_gumbel(bz_engine* e, int32_t max_considered, float gumbel_scale, float maxvisit_init,
                             float value_scale, void* buf, int64_t buf_bytes, void* stream);
/* the considered-visit sequence T[n_considered][k], k = 0 .. sims - 1, of mctx's get_sequence_of_considered_visits (the table
 * bz_engine_set_gumbel uploads; n_considered 1..64, sims 1..BZ_ENGINE_MAX_SIMS).  Host only. */
int32_t bz_gumbel_considered_visits(int32_t n_considered, int32_t sims, uint16_t* out);
/* Gumbel interior selection (the interior rule of Gumbel MuZero, mctx's gumbel_muzero_interior_action_selection),
 * opt-in per engine on top of Gumbel root search: below the root a walk standing at an expanded node X with n > 1 edges takes the
 * first maximum of sc_i = p_i - float(N_i) / (1.0f + float(S)), S = the visit sum of X's children, p = the improved policy of X:
 * softmax(logf(P~_i) + sigma_i) by the sequence of DESIGN.md 3.5 (ascending strict max, expf_spec, sequential sum, division),
 * sigma_i from the "completed Q, sigma" paragraph of DESIGN.md 3.13 on X's current N / W / P with v_root replaced by v_X, the
 * value X was expanded with (the evaluator's, or the one the evaluation cache copied).  n == 1 (a forced pass): edge 0.  No
 * c_puct, no noise below the root; the root rule, expansion, backup, the move, pi' and the rows are those of DESIGN.md 3.13.
 * Combines with everything Gumbel root search combines with.  Searches go through k_gfull_step in place of k_gumbel_step. */
/* bytes of the caller-owned buffer: v_X f32 [n_games][node capacity of a game's arena = sims + 2], rounded up to 256 bytes.
 * Needs no GPU; -1 (bz_last_error says why) for a bad config or a combination Gumbel root search refuses. */
int64_t bz_engine_gumbel_interior_bytes(const bz_engine_cfg* cfg);
/* switch the interior rule on (on != 0) or off (on == 0: k_gumbel_step again), between searches.  BZ_EINVAL (bz_last_error says
 * why) when Gumbel root search is not on, or when buf is null, not 256-byte aligned or smaller than
 * bz_engine_gumbel_interior_bytes.  buf: device memory owned by the caller and kept alive while the rule is on; it needs no
 * initialisation (a node's value is written with its expansion).  bz_engine_set_gumbel(e, 0, ...) switches this off too. */
int32_t bz_engine_set_gumbel_interior(bz_engine* e, int32_t on, void* buf, int64_t buf_bytes, void* stream);
/* the rule for one node on the host, from the functions the kernel runs: N, W, P [n] the edges' visits, value sums (for X's
 * mover) and priors in edge order, n in 1 .. 64, v_node = v_X.  Fills p_out [n] and score_out [n] (either may be null) and
 * returns the chosen edge; -1 (bz_last_error says why) for bad arguments.  Host only. */
int32_t bz_gumbel_interior_pick(const uint32_t* N, const float* W, const float* P, int32_t n, float v_node, float maxvisit_init,
                                float value_scale, float* p_out, float* score_out);
/* Playout cap randomisation (KataGo, Wu 2019, section 3.1), opt-in per engine.  Before every search each
 * slot draws its simulation budget: cfg.sims (a "full" search) when (rng_draw(seed ^ 0x706C61796F757443, game id, moves made)
 * & 0xFFFF) < full_q, else fast_sims -- game id and moves made as the Dirichlet noise keys them.  The slot searches with that
 * budget (its tree is bit for bit that of an engine with sims = budget) and then idles: it uses no evaluator row, while the
 * caller still issues cfg.sims steps.  bz_engine_play records an example row for a full search only; a fast search plays its
 * move by the same rule and writes nothing, so a finished game may have ex_len = 0 (unfinished stays -1) -- the packed block
 * counts such a game in n_games.  Dirichlet noise is drawn on full searches only.  The budgets are drawn by
 * bz_engine_root_begin, so step-API callers need no new call.  Refused combinations: the list at BZ_OPT_*.  Every evaluator and
 * evaluation-cache mode works unchanged.  Searches go through the step kernels. */
/* bytes of the caller-owned buffer: the budgets u32 [n_games] of the current search (0 = the slot took no part), rounded up
 * to 256 bytes.  Needs no GPU; -1 (bz_last_error says why) for a bad config or a refused combination. */
int64_t bz_engine_playout_cap_bytes(const bz_engine_cfg* cfg);
/* switch the cap on (1 <= fast_sims < cfg.sims; full_q in 0 .. 65536 = the probability of a full search in units of 2^-16:
 * 65536 = every search full, 0 = every search fast) or off (fast_sims 0), between searches.  buf: device memory of >=
 * bz_engine_playout_cap_bytes bytes, 256-byte aligned, owned by the caller and kept alive while the mode is on; it is zeroed
 * on `stream`. */
int32_t bz_engine_set_playout_cap(bz_engine* e, int32_t fast_sims, uint32_t full_q, void* buf, int64_t bytes, void* stream);
/* the budget the engine draws for game `gid` at `moves_made` (sims or fast_sims; -1 for bad arguments).  Host only: for tests
 * and for callers who want to predict a game's budgets. */
int32_t bz_playout_cap_budget(uint64_t seed, uint64_t gid, uint32_t moves_made, int32_t sims, int32_t fast_sims, uint32_t full_q);
/* Forced playouts and policy target pruning (KataGo, Wu 2019, section 3.2), opt-in per engine, for self-play.
 * Forced playouts: at the root (depth 0 of a walk) an edge with N > 0 and float(N) < fsqrt((k * P) * float(sum N)) -- P the prior
 * after the Dirichlet noise, sum N the root's child visit sum so far -- scores +inf; the walk takes the first maximum, so the
 * lowest forced action.  Policy target pruning (prune != 0): the pi of the example row and of bz_engine_root_policy is N' / sum N'
 * with the N' of bz_forced_prune below; the move is chosen from the raw N as before, and bz_engine_root_stats
 * reports the raw N.  prune == 0: forcing alone, pi = N / sum N.  Under playout cap randomisation only the full searches force
 * (and only they record).  Refused combinations: the list at BZ_OPT_*.  Also refused (BZ_EINVAL with a message): a negative or
 * non-finite k.  Every evaluator and every evaluation-cache mode work unchanged.  Searches go through the step kernels. */
/* switch forced playouts on (k > 0; KataGo's default is 2.0) or off (k == 0), between searches.  Nothing is uploaded: `stream`
 * is accepted for symmetry with the other setters. */
int32_t bz_engine_set_forced_playouts(bz_engine* e, float k, int32_t prune, void* stream);
/* BZ_OK when an engine of this config accepts bz_engine_set_forced_playouts(e, k, ...), else BZ_EINVAL (bz_last_error says
 * why: a bad config, a refused combination, a bad k).  Needs no GPU.  (It sees the config-carried options only: the setters
 * refuse each other.) */
int32_t bz_engine_forced_playouts_check(const bz_engine_cfg* cfg, float k);
/* Policy target pruning of one root, the function the kernels run.  N, W, P [n]: the root edges' visits, value sums and priors
 * in edge order (ascending action), n in 1 .. 255, N[i] <= 16383, k finite and > 0.  N_out [n]: with c* the first maximum of N
 * and s* its DESIGN.md 3.3 score, every other visited edge loses visits one at a time, up to min(ceil(fsqrt((k * P) *
 * float(sum N))), N), while its score with the reduced N in the u term stays below s*; an edge that lost a visit and is left
 * with <= 1 gets 0; c* and unvisited edges keep theirs.  Host only. */
int32_t bz_forced_prune(const uint32_t* N, const float* W, const float* P, int32_t n, float c_puct, float k, uint32_t* N_out);
/* First-play urgency (FPU) reduction (Leela Zero, LC0, KataGo's fpuReductionMax / rootFpuReductionMax), opt-in per
 * engine: the select rule of DESIGN.md 3.3 scores an edge that was never visited with the value of its parent minus a reduction
 * that grows with the prior mass already explored, instead of with q = 0.  At every level of every walk, for the node X whose
 * edges are scored, every expression one binary32 operation in the written order:
 *   S  = sum over X's edges with N > 0 of (P > 0 ? (u32)(P * 16777216.0f) : 0) -- an exact scaling, a truncating conversion, a
 *        u32 sum (no order, so nothing rounds differently however the lanes reduce it); m = (float)S; m = m * 2^-24; m = fsqrt(m)
 *   qx = below the root: fdiv(W_in, (float)N_in), negated, from the statistics of the edge the walk came in by as the walk read
 *        them (W is stored for the parent's mover; N_in >= 1); at the root: sumN > 0 ? fdiv(Wr, (float)sumN) : 0, sumN = the
 *        simulations done so far in this search and Wr their running sum: 0 at the start of every search, Wr = Wr + x after each
 *        simulation, x = what that simulation's backup added to its root edge's W (one addition per simulation, in simulation
 *        order -- NOT the sum over the root's edges)
 *   f  = qx - (depth == 0 ? root_reduction : reduction) * m;  an edge with N == 0 takes q = f, one with N > 0 keeps fdiv(W, N);
 *        u, s = q + u, the ascending order and the strict first maximum are unchanged.  No clamp: f may be below -1.
 * The Dirichlet noise is in the root's P when the mass is taken.  Both reductions may be 0 (an unvisited child is then worth
 * exactly its parent), which is still not "off".  bz_engine_root_stats, pi = N / sum N, the move choice and the example rows are
 * what they are without it.  Refused combinations: the list at BZ_OPT_*.  Also refused (BZ_EINVAL / -1 with a message): a negative
 * or non-finite reduction.  Under the playout cap fast searches use the rule too; the +inf of a forced edge still wins.  Every
 * evaluator (the external one through the step API included) and every evaluation-cache mode work unchanged.  Searches go through
 * the step kernels. */
/* bytes of the caller-owned buffer: Wr f32 [n_games], rounded up to 256 bytes.  Needs no GPU; -1 (bz_last_error says why) for a
 * bad config or a refused combination. */
int64_t bz_engine_fpu_bytes(const bz_engine_cfg* cfg);
/* BZ_OK when an engine of this config accepts bz_engine_set_fpu(e, 1, reduction, root_reduction, ...), else BZ_EINVAL
 * (bz_last_error says why).  Needs no GPU. */
int32_t bz_engine_fpu_check(const bz_engine_cfg* cfg, float reduction, float root_reduction);
/* switch the rule on (on != 0; reduction, root_reduction finite and >= 0 -- KataGo's defaults are 0.2 and 0.1) or off (on == 0:
 * the plain kernels again), between searches.  buf: device memory of >= bz_engine_fpu_bytes bytes, 256-byte aligned, owned by
 * the caller and kept alive while the mode is on; it is zeroed on `stream`. */
int32_t bz_engine_set_fpu(bz_engine* e, int32_t on, float reduction, float root_reduction, void* buf, int64_t bytes, void* stream);
/* S of one node, the function the kernels run: N, P [n] the edges' visits and priors, n in 1 .. 255, every P <= 2 (or NaN);
 * 0xFFFFFFFF (bz_last_error says why) for bad arguments.  Host only. */
uint32_t bz_fpu_mass(const uint32_t* N, const float* P, int32_t n);
/* f of that node for a node value q_node and a reduction: fpu_value(S, q_node, reduction) as the kernels compute it; NaN for
 * bad arguments.  Host only. */
float bz_fpu_value(const uint32_t* N, const float* P, int32_t n, float q_node, float reduction);
/* Proven wins, losses and draws (MCTS-Solver, Winands et al. 2008; LC0's "certainty propagation"), opt-in per
 * engine.  It runs no second search: it books what the walks of the search already find.
 * State: the edge into a child X is DECIDED with a value c in {-1, 0, +1} for the mover at X -- the convention of the terminal
 *   value an edge already stores.  An edge into a terminal child is decided from its creation; another edge becomes decided by
 *   the proof pass (bit 30 of the edge's word 0, the value in the bits of the terminal value).  An edge without a child, and
 *   every edge an expansion, an evaluation-cache copy or the root store writes, is undecided: a cached evaluation carries priors
 *   and a value, never a proof.
 * Node rule, for a node X with n edges of decided values c_i: X is decided +1 as soon as some c_i = -1; otherwise X is decided
 *   only when all n edges are decided, with max over i of -c_i.  The colours alternate on every edge, passes included: a pass
 *   node (n = 1) is decided exactly when its child is.  All of it is integer: bz_solver_node is the function the kernels run.
 * Backup: when the leaf of a backup was terminal or a decided edge, the node rule runs on the block of edges the deepest path edge
 *   lies in; a decided parent marks the path edge into it and the pass goes on one level up; it stops at the first undecided
 *   parent, at the root -- whose value is recorded per game in the caller's buffer -- and proves nothing on a path longer than
 *   the engine's depth limit.  The backup of an evaluated leaf is untouched.
 * Select: the scores of DESIGN.md 3.3 with (a) an edge decided c = -1 (the move wins) scoring +inf, (b) an edge decided c = +1
 *   scoring -inf -- edge 0 when every edge does -- and (c) an edge decided c = 0 taking q = 0 exactly, its u unchanged; ascending
 *   order and the strict first maximum as before.  A walk that takes a decided edge ends there with value c and needs no
 *   evaluator row: no walk passes a decided edge, and the root's visits still sum to the simulations.
 * Move (bz_engine_play, bz_engine_root_policy; bz_solver_pick is the function): the lowest root edge decided c = -1 at every
 *   temperature; otherwise the rule of DESIGN.md 3.7 over the edges not decided c = +1 (sampling: the draw modulo THEIR visit
 *   sum); when every edge is decided +1 or the remaining visit sum is 0, over all edges.  The recorded pi stays N / sum N.
 * Refused combinations: the list at BZ_OPT_*.  Every evaluator (the external one through the step API) and every evaluation-cache
 * mode work unchanged.  Searches go through the step kernels. */
/* bytes of the caller-owned buffer: the roots' values i32 [n_games] and two u32 counts, each rounded up to 256 bytes.  Needs no
 * GPU; -1 (bz_last_error says why) for a bad config or a refused combination. */
int64_t bz_engine_solver_bytes(const bz_engine_cfg* cfg);
/* BZ_OK when an engine of this config accepts bz_engine_set_solver(e, 1, ...), else BZ_EINVAL.  Needs no GPU. */
int32_t bz_engine_solver_check(const bz_engine_cfg* cfg);
/* switch the solver on (on != 0) or off (on == 0: the plain kernels again), between searches.  buf: device memory of >=
 * bz_engine_solver_bytes bytes, 256-byte aligned, owned by the caller and kept alive while the mode is on; zeroed on `stream`
 * here and by every bz_engine_root_begin. */
int32_t bz_engine_set_solver(bz_engine* e, int32_t on, void* buf, int64_t bytes, void* stream);
/* the proof state after a search, into device memory: edge_out int8 [n_games][NA], the decided value of the root edge of every
 * action (2: undecided, or no such edge); root_out int8 [n_games], the root's recorded value (2: undecided); counts_out
 * uint32 [2]: nodes newly decided in this search (roots included), walks that ended at a decided edge that is not terminal. */
int32_t bz_engine_root_proven(bz_engine* e, int8_t* edge_out, int8_t* root_out, uint32_t* counts_out, void* stream);
/* the node rule: vals [n] in {-1, 0, +1, 2 = undecided}, n in 1 .. 255; returns the node's value or 2; -128 for bad arguments.
 * Host only. */
int32_t bz_solver_node(const int8_t* vals, int32_t n);
/* the move rule: N, vals [n] the root edges' visits and decided values, tau1 != 0: sampling with the 64-bit draw, else the
 * first maximum; returns the edge index; -1 for bad arguments.  Host only. */
int32_t bz_solver_pick(const uint32_t* N, const int8_t* vals, int32_t n, int32_t tau1, uint64_t draw);
/* Exact early stop ("early stop" of Huang, Coulom and Lin 2010 and Baier and Winands 2012, LC0's "smart
 * pruning" without its slack), opt-in per engine, for the searches whose move is the first maximum of the root's visits.
 * Rule (bz_early_stop_decided is the function the kernels run; all of it is integer): the root has n edges in ascending action
 *   order with visits N_i, s = sum N_i simulations are done and left = sims - s are to go; L is the first maximum of N.  The
 *   search is DECIDED when s >= 1 and every j != L has N_j + left < N_L, or N_j + left == N_L and j > L (a tie goes to the lower
 *   action).  Visits never decrease and the remaining simulations add at most `left` to one edge, so a decided search plays the
 *   move the full search plays.  left = 0 is always decided, a one-edge root at s = 1, and with n >= 2 nothing before s >= left:
 *   at most half of a search is saved.
 * Where: in the tree step of simulation index s (1 <= s < sims), behind its expansion and backup and in front of its walk.  A
 *   decided slot selects nothing, is left without a leaf, records stop_at = s and is idle for the rest of the search, like a
 *   slot at its playout-cap budget.  A slot whose move is sampled (moves made < temp_moves) never stops.
 * For every observer a stopped search is a full search: its row is recorded, and bz_engine_root_policy, bz_engine_root_stats
 *   and bz_engine_play see the tree as it stands (pi = N / stop_at).
 * Host exit (host_exit != 0): bz_engines_search with run_ahead_sims > 0 ends an engine's step loop as soon as a completed
 *   run-ahead mark shows that no slot of the engine walks any more -- no launch and no wait is added, the results are the same
 *   bits, only empty launches are saved.  bz_engine_search and bz_engines_step run every step.
 * Refused combinations: the list at BZ_OPT_*.  temp_moves, every evaluator (the external one through the step API) and every
 * evaluation-cache mode work unchanged.  Searches go through the step kernels. */
/* bytes of the caller-owned buffer: stop_at u32 [n_games] and one u32 word, each rounded up to 256 bytes.  Needs no GPU; -1
 * (bz_last_error says why) for a bad config or a refused combination. */
int64_t bz_engine_early_stop_bytes(const bz_engine_cfg* cfg);
/* BZ_OK when an engine of this config accepts bz_engine_set_early_stop(e, 1, ...), else BZ_EINVAL.  Needs no GPU. */
int32_t bz_engine_early_stop_check(const bz_engine_cfg* cfg);
/* switch early stop on (on != 0) or off (on == 0: the plain kernels again), between searches.  buf: device memory of >=
 * bz_engine_early_stop_bytes bytes, 256-byte aligned, owned by the caller and kept alive while the mode is on; zeroed on
 * `stream` here, reset by every bz_engine_root_begin. */
int32_t bz_engine_set_early_stop(bz_engine* e, int32_t on, int32_t host_exit, void* buf, int64_t bytes, void* stream);
/* stop_at of the last search into device memory, uint32 [n_games]: the simulations the slot's search ran -- cfg.sims when it ran
 * its whole budget, 0 for a slot that sat the search out. */
int32_t bz_engine_stopped(bz_engine* e, uint32_t* out, void* stream);
/* the rule: N [n] the root edges' visits (each < 2^24) in ascending action order, n in 1 .. 255, left the simulations to go;
 * returns 1 (decided) or 0; -1 for bad arguments.  Host only. */
int32_t bz_early_stop_decided(const uint32_t* N, int32_t n, uint32_t left);

/* ---- The replay seed.  After a move the new root is a child of the old one, and a fresh search from it
 * re-creates that child's old subtree node for node for its first N_e - 1 simulations (N_e = the played edge's visits).  Where the
 * carry-over is on and the search is otherwise plain (no other search mode, no noise, no subtree reuse, no evaluation symmetry;
 * bz_engine_search / bz_engines_search / bz_engines_step), every such slot starts from a copy of that subtree instead and makes its
 * remaining r = sims - (N_e - 1) walks in the launches bz_pace_walk names, so that the move's launches carry even row counts.
 * No result and no counter changes.  bz_engine_set_replay_seed: mode 0 = off, 1 = on, 2 (the default) = on for an engine of more
 * than 1024 slots -- below that a launch's time does not follow its rows and level launches cost more than they save.
 * bz_pace_walk: walk[L] = 1 iff a slot with r walks left walks in launch L of 0 .. sims - 1, done[L] = its walks before launch L:
 * floor((L + 1) r / sims) > floor(L r / sims), and floor(L r / sims). */
int32_t bz_engine_set_replay_seed(bz_engine* e, int32_t mode);
int32_t bz_pace_walk(int32_t sims, int32_t r, uint8_t* walk, uint32_t* done);
/* Policy surprise weighting (KataGo, Wu 2019, section 3.3), opt-in per engine.  Every row bz_engine_play
 * records gets kl = sum over the root's edges in ascending action order with pi_a > 0 of pi_a * (logf(pi_a) - logf(max(P_a,
 * FLT_MIN))), every operation one binary32 operation, then kl > 0 ? kl : 0 (a rounding negative or a NaN: 0).
 * pi = the row's recorded pi, whatever produced it (N / sum N, the pruned target of 3.16, Gumbel's improved policy); P = the
 * root's raw prior as the expansion stored it, before the Dirichlet noise.  The feature observes: searches, moves, pi and the
 * example arrays are what they are without it, and bz_engine_layout does not change.  With cfg.dirichlet_eps > 0
 * bz_engine_root_noise saves the priors in front of the noise; without noise nothing ever rewrites a prior, and bz_engine_play
 * saves them from the searched root -- so step-API callers need no new call, and every search runs the kernels it runs with the
 * mode off (the fused single-launch searches included: the work counters stay the same too).  bz_engine_play notes the row in
 * front of its play kernel and computes the kl behind it (a fast search under the playout cap records no row and no kl).
 * Nothing the engine accepts is refused: PUCT, leaves_per_step > 1, subtree reuse, Gumbel, the cap, forced playouts, every
 * evaluator and evaluation-cache mode. */
/* bytes of the caller-owned buffer: the saved raw priors f32 [n_games][MAXCH] (34 Reversi, 9 tic-tac-toe; edge order), a
 * pending-row word u64 [n_games] and ex_kl f32 [rounds][n_games][t_max] (the row index of ex_pi), each 256-byte aligned.
 * Needs no GPU; -1 (bz_last_error says why) for a bad config. */
int64_t bz_engine_surprise_bytes(const bz_engine_cfg* cfg);
/* switch the mode on (buf: device memory of >= bz_engine_surprise_bytes bytes, 256-byte aligned, owned by the caller and kept
 * alive while the mode is on; zeroed on `stream`) or off (buf == NULL), between searches. */
int32_t bz_engine_set_surprise(bz_engine* e, void* buf, int64_t bytes, void* stream);
/* ex_kl in the packed block's row order: out f32 [cap_rows], row r of the block bz_engine_pack_examples has just filled gets
 * its kl.  Call it after that bz_engine_pack_examples, on the same stream, with the same cap_rows: it uses the per-game row
 * offsets that call left, which already count the rows earlier engines appended -- so the second pipeline of a rank lands
 * behind the first.  append_rows (>= 0): the rows already in `out`, 0 for the first engine; they are left alone.  Games that
 * did not fit into the block stay out of `out` too. */
int32_t bz_engine_pack_surprise(bz_engine* e, float* out, int64_t cap_rows, int32_t append_rows, void* stream);
/* the kl of one row, the function the kernels run: pi, P [n] in edge order, n in 1 .. 255.  Host only. */
int32_t bz_surprise_kl(const float* pi, const float* P, int32_t n, float* kl);
/* From surprise to repeat counts: rows are repeated in the data, not reweighted in the loss.  Device only,
 * asynchronous, nothing read back.  kl f32, game i64, ply i32, own / opp u64 [n]: the rows (n <= 2^26, else BZ_EINVAL).
 *   mean = float(double(sum_i (u64)(kl_i * 2^30)) / (double(n) * 2^30)): an exact 64-bit integer sum, the same bits every run
 *          (kl_i is first cleaned: negative or NaN -> 0, above 128 -> 128)
 *   w_i = uniform_frac + (1 - uniform_frac) * (kl_i / mean), single binary32 operations, uniform_frac in [0, 1] (KataGo: 0.5);
 *         mean == 0: w_i = 1; w_i is capped at 2^30
 *   count_i = floor(w_i) + [draw_i < (u32)(frac(w_i) * 2^24)], draw_i = mix64(rng_draw(seed ^ 0x7375727072697365, game_i,
 *         ply_i) ^ hash_pos(own_i, opp_i)) >> 40: keyed by the row's content, not by its index
 * count i32 [n] gets the counts; idx_out i64 [idx_cap] row i repeated count_i times, ascending; *n_out (device i64) =
 * min(sum count, idx_cap).  Entries beyond idx_cap are dropped and counted: the workspace starts with three u64 words -- the
 * integer kl sum, sum count and the number of dropped entries -- that the caller may read once the stream has run.
 * ws: bz_surprise_resample_workspace_bytes(n) bytes, 256-byte aligned. */
int64_t bz_surprise_resample_workspace_bytes(int64_t n);
int32_t bz_surprise_resample(const float* kl, const int64_t* game, const int32_t* ply, const uint64_t* own, const uint64_t* opp,
                             int64_t n, float uniform_frac, uint64_t seed, void* ws, int64_t ws_bytes, int32_t* count,
                             int64_t* idx_out, int64_t idx_cap, int64_t* n_out, void* stream);
/* count_i of one row, the function the kernels run.  Host only. */
int32_t bz_surprise_count(float kl, float mean, float uniform_frac, uint64_t seed, int64_t game, int32_t ply, uint64_t own,
                          uint64_t opp, int32_t* count);
/* Search-value targets, opt-in per engine.  Every row bz_engine_play records also gets the root's search
 * value q: over the root's edges in edge order (ascending action) sW = 0.0f, sW = sW + W_i (one binary32 add each), sN = sum
 * N_i (integer), q = sN > 0 ? fdiv(sW, (float)sN) : 0.0f.  W is stored for the mover at the root: q is the
 * mover's expected outcome.  Always the RAW visit statistics: under Gumbel, under forced playouts (not the pruned visits), with
 * subtree reuse (carried visits included) and with leaves_per_step > 1 (no virtual loss is left after a search).  The feature
 * observes: bz_engine_play launches one one-lane-per-game kernel in front of its play kernel, while the searched tree is in
 * place -- so it does not depend on how the search ran (fused, step kernels, the step API), and searches, rows, counters and
 * bz_engine_layout are what they are without it.  A fast search under the playout cap records no row and no q. */
/* bytes of the caller-owned buffer: ex_q f32 [rounds][n_games][t_max] (the row index of ex_pi), 256-byte aligned.  Needs no
 * GPU; -1 (bz_last_error says why) for a bad config. */
int64_t bz_engine_search_value_bytes(const bz_engine_cfg* cfg);
/* switch the mode on (buf: device memory of >= bz_engine_search_value_bytes bytes, 256-byte aligned, owned by the caller and
 * kept alive while the mode is on; zeroed on `stream`) or off (buf == NULL), between searches. */
int32_t bz_engine_set_search_value(bz_engine* e, void* buf, int64_t bytes, void* stream);
/* ex_q in the packed block's row order: bz_engine_pack_surprise's contract (after bz_engine_pack_examples, same stream, same
 * cap_rows; append_rows: the rows already in `out`). */
int32_t bz_engine_pack_search_value(bz_engine* e, float* out, int64_t cap_rows, int32_t append_rows, void* stream);
/* q of one root, the function the kernel runs: N, W [n] in edge order, n in 1 .. 255.  Host only. */
int32_t bz_root_value(const uint32_t* N, const float* W, int32_t n, float* q);
/* Value targets from (q, z) (TD(lambda): Sutton 1988).  Device only, asynchronous, nothing read back.  q f32, z
 * i8, mover i8 (+-1), game i64, ply i32 [n]: the rows, n <= 2^26; lam, q_mix in [0, 1] (anything else, NaN included: BZ_EINVAL
 * before a launch).  Row i starts a segment iff i == 0, game[i] != game[i-1] or ply[i] <= ply[i-1]: a segment is one game's
 * recorded rows in ply order (what the packed block delivers).  Per segment of T rows, every line one binary32 operation:
 *   c_t = q_t != q_t ? 0 : clamp(q_t, -1, 1);  A_t = mover_t == 1 ? c_t : -c_t;  Z = (float)(mover_{T-1} * z_{T-1})
 *   G_{T-1} = Z;  for t = T-2 .. 0:  a = 1 - lam; a = a * A_{t+1}; b = lam * G_{t+1}; G_t = a + b
 *   c = 1 - q_mix; c = c * G_t; d = q_mix * A_t; T_t = clamp(c + d, -1, 1);  vt_t = mover_t == 1 ? T_t : -T_t
 * lam = 1, q_mix = 0: vt == (float)z by value; lam = 0, q_mix = 1: vt == the cleaned q.  One lane per segment walks it
 * backward, at most 1024 rows (the engine's segments have at most 256): a longer segment gets vt = (float)z on all its rows
 * and adds 1 to *status_dev, a u64 word in device memory that the call zeroes first and the caller may read once the stream
 * has run.  vt f32 [n]. */
int32_t bz_value_targets(const float* q, const int8_t* z, const int8_t* mover, const int64_t* game, const int32_t* ply, int64_t n,
                         float lam, float q_mix, float* vt, uint64_t* status_dev, void* stream);
/* one segment, the function the kernel runs: q, z, mover, vt [T], T in 1 .. 1024.  Host only. */
int32_t bz_value_targets_segment(const float* q, const int8_t* z, const int8_t* mover, int32_t T, float lam, float q_mix, float* vt);
/* Position averaging (AlphaZero.jl's use_position_averaging): the rows of a window that share a position --
 * exactly equal (own, opp) -- become one row with the mean pi, the mean value target and a count.  All sums are integer sums of
 * fix_k(x) = (int64)(x * 2^k) (truncating; the product is exact in binary32): k = 32 for pi in [0, 1] and for the value input,
 * q in [-1, 1]; k = 24 for kl in [0, 128].  The value input of a row is vt[i] when vt is given, else (float)z[i].  A group of n
 * rows with sum S gives M = floor((2 S + n) / (2 n)) (integers: round half up, a true floor for negative S) and the result
 * (float)((double)M * 2^-k).  n == 1: the row itself bit for bit, vt = its value input.  z = sign(the value sum).  A row holding
 * a value that is NaN or outside its range adds to no sum and is counted; n stays the group's number of rows. */
typedef struct bz_merge_rows {  /* the columns of n rows (input) or of the merged rows (output); q and kl may be NULL */
    uint64_t* own; uint64_t* opp; float* pi; int8_t* z; int8_t* mover; uint8_t* act; int64_t* game; int32_t* ply;
    float* vt;  /* input: NULL = the value input is (float)z; output: never NULL */
    float* q; float* kl;
} bz_merge_rows;
/* one group, the function the kernels run: pi [n][na], z [n], vt / q / kl [n] or NULL; n in 1 .. 2^26, na 9 or 65.  *bad = the
 * rows that were not summed.  Host only. */
int32_t bz_merge_group(const float* pi, const float* vt, const int8_t* z, const float* q, const float* kl, int32_t n, int32_t na,
                       float* pi_out, float* vt_out, int8_t* z_out, float* q_out, float* kl_out, int32_t* bad);
/* bytes of bz_merge_positions' workspace: one row of na + 3 int64 sums per possible group, 256-byte aligned.  -1 for n outside
 * 0 .. 2^26 or na not 9 / 65.  Needs no GPU. */
int64_t bz_merge_workspace_bytes(int64_t n, int32_t na);
/* Device only, asynchronous, nothing read back.  The caller has grouped the rows (two stable sorts make equal positions
 * adjacent with the first occurrence in front): per sorted position i, order[i] = the row standing there, start[i] = the sorted
 * position of the head of its run, dst[i] = the output row of its group (groups numbered by first occurrence in the input); per
 * output row d < *n_groups (a device word), head[d] = the group's first row and count[d] = its rows.  Output row d gets the
 * merged pi, vt, z (and q, kl when the input has them) and the head's own, opp, mover, act, game, ply.  *status_dev, a u64 word
 * in device memory that the call zeroes first, counts the rows that were not summed (and the entries of order / dst outside
 * 0 .. n-1, which are never followed).  n == 0: nothing is launched and no pointer is looked at. */
int32_t bz_merge_positions(const bz_merge_rows* in, int64_t n, int32_t na, const int64_t* order, const int32_t* start,
                           const int32_t* dst, const int64_t* head, const int32_t* count, const int64_t* n_groups, void* ws,
                           int64_t ws_bytes, const bz_merge_rows* out, uint64_t* status_dev, void* stream);
/* Ownership targets (KataGo, Wu 2019, section 5), opt-in per engine.  When a move of bz_engine_play ends a
 * game, the position that move produced is kept in absolute colours: fin_x = the stones of X (the side that moves with
 * to_move = +1), fin_o = O's, u64 [rounds][n_games] each, indexed like ex_len, in the engine's bit layout.  Valid iff
 * ex_len >= 0, 0 otherwise (bz_engine_reset_games zeroes them).  A game that records no row (every search fast under the
 * playout cap) still records its final board.  The feature observes: bz_engine_play launches the kernel behind
 * bz_engine_root_policy (into scratch inside the buffer) and one one-lane-per-game kernel in front of its play kernel, while
 * the searched tree is in place -- searches, rows, counters and bz_engine_layout are what they are without it. */
/* bytes of the caller-owned buffer: fin_x, fin_o u64 [rounds][n_games], then the scratch pi f32 [n_games][NA] and act i32
 * [n_games], each 256-byte aligned.  Needs no GPU; -1 (bz_last_error says why) for a bad config. */
int64_t bz_engine_ownership_bytes(const bz_engine_cfg* cfg);
/* switch the mode on (buf: device memory of >= bz_engine_ownership_bytes bytes, 256-byte aligned, owned by the caller and
 * kept alive while the mode is on; zeroed on `stream`) or off (buf == NULL), between searches. */
int32_t bz_engine_set_ownership(bz_engine* e, void* buf, int64_t bytes, void* stream);
/* the rows' target boards in the packed block's row order, two u64 per row (bz_ownership_row of the row's game and the row's
 * ex_mover): bz_engine_pack_surprise's contract (after bz_engine_pack_examples, same stream, same cap_rows; append_rows: the
 * rows already in the arrays). */
int32_t bz_engine_pack_ownership(bz_engine* e, uint64_t* fown_out, uint64_t* fopp_out, int64_t cap_rows, int32_t append_rows,
                                 void* stream);
/* a row's target boards, the function the kernel runs: *t_own = mover == +1 ? fin_x : fin_o, *t_opp = the other board; the
 * target of cell i is bit_i(t_own) - bit_i(t_opp) in {+1, 0, -1}.  mover: +1 or -1.  Host only. */
int32_t bz_ownership_row(uint64_t fin_x, uint64_t fin_o, int32_t mover, uint64_t* t_own, uint64_t* t_opp);
/* Resignation in self-play (AlphaGo Zero, Silver et al. 2017, "Self-play"), opt-in per engine.  After a search
 * and before its move, q = the root's sum W / sum N for the mover (bz_root_value on the raw statistics bz_engine_root_stats
 * reports, whatever the search mode: the bits of 3.18's ex_q).  Every game keeps one streak per side, 0 at its start: a FULL
 * search (under playout cap randomisation a fast one touches nothing) sets the mover's streak to min(streak + 1, 255) if
 * q < threshold (strict, binary32; a NaN q is not below it) and to 0 otherwise, and the side FIRES when its streak has
 * reached `consecutive`.  A pass is no search and touches nothing.  The first fire of a game writes its record: the side
 * (+1 / -1), the moves made and q.  A game is PLAYED OUT iff
 *     (rng_draw(seed ^ BZ_RESIGN_KEY, gid, 0) & 0xFFFF) < playout_q,   gid = game_id_base + round x game_id_stride + slot
 * -- a function of (seed, gid) alone -- and then goes on as if nothing had happened: the record is the only trace, and the
 * game's real outcome says whether the resignation would have been right.  Any other game ends at its first fire: the firing
 * search records no row and plays no move, the other side wins, z is back-filled over the rows recorded so far, ex_len,
 * ex_winner and the finished-games count follow, and with `restart` and a round left the slot starts its next game.  Such a
 * game's rows are a prefix of the rows it has without resignation; a game may end with ex_len = 0.
 * bz_engine_play then launches k_resign_note first (one lane per game: q, the streak, the record, a resigning game's end; the
 * slot leaves the active state, so every later kernel of the play skips it by the test it already makes) and k_resign_finish
 * last (restart or retire the resigned slots).  Off (the default) launches nothing and changes no bit. */
#define BZ_RESIGN_KEY 0x72657369676E6564ULL /* "resigned" */
/* bytes of the caller-owned buffer: streaks u8 [rounds][n_games][2] (side +1, side -1), then per game [rounds][n_games],
 * indexed like ex_len: side i8 (0 = no record), moves made i32, q f32, played out u8 -- each array 256-byte aligned.  Needs no
 * GPU; -1 (bz_last_error says why) for a bad config. */
int64_t bz_engine_resign_bytes(const bz_engine_cfg* cfg);
/* on (buf: device memory of >= bz_engine_resign_bytes bytes, 256-byte aligned, owned by the caller and kept alive while the
 * mode is on; zeroed on `stream`, as bz_engine_reset_games does) or off (buf == NULL: no extra launch), between searches.
 * Called again with the buffer the engine already uses it only changes threshold, consecutive and playout_q: streaks and
 * records stay.  threshold: finite, in [-1, 1]; consecutive in 1 .. 255; playout_q in 0 .. 65536.  Refused (BZ_EINVAL,
 * bz_last_error names this function) for a null engine, an unaligned or too small buffer, a bad argument, and together with
 * ownership targets -- in either order of the two setters: a resigned game has no final board. */
int32_t bz_engine_set_resign(bz_engine* e, float threshold, int32_t consecutive, uint32_t playout_q, void* buf, int64_t bytes,
                             void* stream);
/* copies of the records into device arrays of [rounds][n_games] elements each: side i8, moves made i32, q f32, played out u8
 * (written for every game that has had a play) */
int32_t bz_engine_resign_rows(bz_engine* e, int8_t* side, int32_t* move, float* q, uint8_t* played_out, void* stream);
/* the streak rule, the function the kernel runs: *streak_out = the streak behind a full search with root value q; returns 1
 * if the side fires, 0 if not, -1 for a null pointer, consecutive outside 1 .. 255 or streak_in outside 0 .. 255.  Host only. */
int32_t bz_resign_step(float q, float threshold, int32_t consecutive, int32_t streak_in, int32_t* streak_out);
/* 1 if the game with global id gid is played out, 0 if not, -1 for playout_q > 65536: the draw the kernel makes.  Host only. */
int32_t bz_resign_playout(uint64_t seed, uint64_t gid, uint32_t playout_q);
/* The root store, opt-in per engine, active only where the engine runs the carry-over cache
 * (BZ_ENGINE_EVAL_CACHE | BZ_ENGINE_EVAL_CACHE_CARRY with a net evaluator, one leaf per step, no subtree reuse).  The first
 * searches of a game repeat searches other games of the engine already ran: a finished search whose root lies fewer than
 * `plies` moves behind the game's start (the two fixed opening plies not counted) is filed under its root position, `entries`
 * of them at most, and a slot whose next root is on file gets that tree as its "previous search" before bz_engine_root_begin
 * -- the carry-over then shares its evaluations exactly as it shares those of the slot's own previous search, each hit
 * confirmed against the stored position.  Results are bit for bit those without the store; counters[7] drops, counters[8] and
 * [9] rise by as much.  counters[11] = evaluations taken from a seeded tree (part of counters[9]), counters[12] = searches
 * that were seeded, counters[13] = trees filed.  A change of evaluator (bz_net_update, bz_engine_set_net,
 * bz_engine_set_eval_symmetry) empties the store at the next search.
 * Bytes: 256 + 4 x n_idx (n_idx = the power of two >= max(16, 2 x entries)) + 64 x entries + 4 x n_games, then per entry one
 * slot's arenas: nodes 32 x (sims + 2), edges 16 x (sims + 2) x MAXCH (34 on the Reversi boards), node values 4 x (sims + 2)
 * and the slot's table 128 x buckets (buckets = the power of two >= max(16, (sims + 2) / 4)), each array 256-byte aligned --
 * 0.50 MB per entry at 800 simulations.  0 when the config does not run the carry-over cache; -1 for a bad config. */
int64_t bz_engine_root_store_bytes(const bz_engine_cfg* cfg, int32_t entries, int32_t plies);
/* on (buf: device memory of >= bz_engine_root_store_bytes bytes, 256-byte aligned, owned by the caller and kept alive while
 * the store is on; its index is zeroed on `stream`) or off (buf == NULL), between searches.  On an engine without the
 * carry-over cache the call succeeds and the store stays off. */
int32_t bz_engine_set_root_store(bz_engine* e, void* buf, int64_t bytes, int32_t entries, int32_t plies, void* stream);
/* the pi and the action bz_engine_play would write and play, for every slot, after a search: device arrays pi f32
 * [n_games][NA] and action i32 [n_games].  PUCT: pi = N / sum N and the DESIGN.md 3.7 rule (tau = 1 sampling included);
 * Gumbel: the improved policy and the Gumbel move.  Idle or finished slots get pi = 0 and action -1. */
int32_t bz_engine_root_policy(bz_engine* e, float* pi, int32_t* action, void* stream);
/* Reanalysis: stored example rows in, fresh targets out, around one search (bz_engine_search /
 * bz_engines_search) of the positions they hold.  own / opp / mover: the caller's example columns, device arrays [n_rows]
 * (side-to-move canonical bitboards, the mover's absolute colour +1 / -1); rows: device i64 indices into them or NULL = the
 * identity (rows holds at least first + count of them); slot g < count serves row r = rows ? rows[first + g] : first + g, every
 * index in 64-bit arithmetic.
 * bz_engine_reanalyse_load is bz_engine_set_roots from those columns: slot g < count becomes a fresh root at row r (boards,
 * to_move = mover[r], moves / round / passes / rows 0, nothing kept from an earlier search), slots count .. n_games - 1 are
 * idle.  A row outside 0 .. n_rows - 1 leaves its slot idle and raises BZ_ENGINE_ERR_REANALYSE_ROW; nothing is read or
 * written at it.  clear != 0 resets the sticky error word and the eval counters as bz_engine_set_roots does; clear == 0 keeps
 * them, so that one bz_engine_status behind the last chunk reports every chunk.
 * bz_engine_reanalyse_store, behind the search: pi[r * NA ..] = the pi bz_engine_root_policy reports for the slot (N / sum N,
 * the Gumbel improved policy, the pruned pi of forced playouts, the solver's), and where the pointers are not NULL q[r] =
 * bz_root_value of the root's raw statistics and kl[r] = bz_surprise_kl of that pi against the root edges' priors (raw: the
 * caller searches without noise).  Idle slots, terminal roots (BZ_ENGINE_ERR_TERMINAL_ROOT) and unexpanded roots write nothing.
 * Slots that name the same row write the same bits.  BZ_EINVAL for a null engine, a null own / opp / mover / pi, count
 * outside 0 .. n_games, a negative first or n_rows. */
int32_t bz_engine_reanalyse_load(bz_engine* e, const uint64_t* own, const uint64_t* opp, const int8_t* mover, int64_t n_rows,
                                 const int64_t* rows, int64_t first, int32_t count, int32_t clear, void* stream);
int32_t bz_engine_reanalyse_store(bz_engine* e, float* pi, float* q, float* kl, int64_t n_rows, const int64_t* rows,
                                  int64_t first, int32_t count, void* stream);
/* synchronises the stream; number of active slots / finished games so far.  error_flags (sticky until the next
 * reset_games / set_roots): 1 = a game's edge arena overflowed, 2 = a root position was already terminal, 4 = more example
 * rows than t_max, 8 = a walk deeper than the path buffer, 16 = the evaluator returned a non-finite logit or value (the
 * search results of that move are meaningless), 32 = a reanalysed row index outside the caller's columns */
#define BZ_ENGINE_ERR_REANALYSE_ROW 32
#define BZ_ENGINE_ERR_EDGE_OVERFLOW 1
#define BZ_ENGINE_ERR_TERMINAL_ROOT 2
#define BZ_ENGINE_ERR_EXAMPLE_OVERFLOW 4
#define BZ_ENGINE_ERR_DEPTH 8
#define BZ_ENGINE_ERR_EVAL_NONFINITE 16
int32_t bz_engine_status(bz_engine* e, void* stream, int32_t* n_active, int64_t* games_finished,
                         int32_t* error_flags);
/* ------------------------------------------------------------------------ */
/* Packed examples: the rows of the FINISHED games only, compacted on the    */
/* device in (round, slot, ply) order -- the batched form of what            */
/* collect_game_data keeps, src/tic_tac_toe/SL/generate_training_games.py:   */
/* 30-36 (only complete games reach all_states / all_actions).  This is what */
/* the iteration-end all-gather ships (one fixed-capacity buffer per rank).  */
/*                                                                           */
/* Block = 256-byte header, then eight arrays of cap_rows elements, each     */
/* starting at a multiple of 256 bytes:                                      */
/*   header u64[32]: magic 0x425A50414B000001, n_rows, n_games, cap_rows,    */
/*                   NA, game, dropped_rows, bytes, offs[8]                  */
/*   own u64, opp u64, pi f32[NA], game id i64, z i8, mover i8, act u8,      */
/*   ply u8                                                                  */
/* dropped_rows = rows of finished games that did not fit (0 in a healthy    */
/* run; ~0 = an append met a block of another geometry -- it stays: that     */
/* append and every later APPEND write no row and keep n_rows, n_games and   */
/* the ~0, whatever geometry they bring; a pack with append == 0 starts the  */
/* block afresh, which is how a caller recovers the buffer); rows            */
/* [0, n_rows) of every array are valid.                                     */
/* ------------------------------------------------------------------------ */
#define BZ_PACKED_MAGIC 0x425A50414B000001ULL
int64_t bz_examples_packed_bytes(int32_t na, int64_t cap_rows);
/* packed: caller-owned device block of >= bz_examples_packed_bytes(NA, cap_rows) bytes, 256-byte aligned.
 * append == 0: start the block (header + this engine's rows); append != 0: add this engine's rows behind
 * those already there (the second pipeline of a rank).  Asynchronous on `stream`; calls that fill one block
 * must be ordered (same stream, or events). */
int32_t bz_engine_pack_examples(bz_engine* e, void* packed, int64_t packed_bytes, int64_t cap_rows, int32_t append,
                                void* stream);

/* aliases under the names SURVEY.md 8(b) lists: select / expand+backup of one simulation, and
 * one whole move (search + play) for every active slot */
int32_t bz_mcts_select(bz_engine* e, uint32_t sim_index, void* stream);
int32_t bz_mcts_expand_backup(bz_engine* e, void* stream);
int32_t bz_selfplay_run(bz_engine* e, int32_t restart, void* stream);
/* one move (search + play) for n engines -- the pipelines of one GPU, engine i on streams[i] -- issued by ONE host
 * thread and interleaved simulation by simulation.  run_ahead_sims > 0 bounds how far the thread runs ahead of the
 * streams (it then sleeps on blocking-sync events instead of spinning on a full queue; 0 = unbounded, the behaviour of
 * bz_selfplay_run called engine by engine).  Results are those of bz_selfplay_run on every engine.  All engines must
 * search the same number of simulations; n <= 16. */
int32_t bz_engines_step(bz_engine* const* engines, void* const* streams, int32_t n, int32_t restart,
                        int32_t run_ahead_sims);
int32_t bz_engine_reset_counters(bz_engine* e, void* stream);
/* fold the kernels' per-wave counter slots into the layout's counters array (async): words 0..9.  Words 10 (n_collisions) and
 * 11..13 (the root store's) are added to in place by their kernels; 14 and 15 are unused, 16..23 belong to diagnostic builds */
int32_t bz_engine_sum_counters(bz_engine* e, void* stream);

/* ------------------------------------------------------------------------ */
/* Head-to-head match between two search players: B games   */
/* over the same B slots of TWO engines, one per side (A and B), colours     */
/* swapped inside every pair of games.  The turn loop is the one of          */
/*   ReversiTerminal.play  reversi_terminal.py:16-38 (pass rule :31-35)      */
/*   TicTacToeHeadless.play  src/tic_tac_toe/tic_tac_toe.py:13-34            */
/* with a search player on both sides.  Everything between two searches is   */
/* ONE kernel per ply (csrc/bz_match.hip) and the host reads 32 bytes.       */
/*                                                                           */
/* Per ply the caller runs                                                   */
/*   bz_engine_set_roots(A, ws + own, ws + opp, ws + to_move_a)   (B alike)  */
/*   a search of every engine whose side has a slot to move                  */
/*   bz_engine_root_policy(A, ., act_a)                           (B alike)  */
/*   bz_match_ply(m, act_a, act_b, A, B)      bz_match_header(m, ., &h)      */
/* until h.n_active == 0 (or h.error != 0).                                  */
/* Games 2k and 2k+1 are a pair: the same opening, A plays +1 (X, moves      */
/* first) in game 2k and -1 in game 2k+1.  While a slot has made fewer than  */
/* opening_plies moves its move is the r-th legal move in ascending action   */
/* order, r = bz_match_opening_index(seed, k, moves made, n_legal); neither  */
/* engine searches the slot then.  A side without a move in an unfinished    */
/* game is passed over (the other side moves again; a pass is no ply), so    */
/* every active slot makes exactly one move per ply.                         */
/* ------------------------------------------------------------------------ */
typedef struct bz_match bz_match;
#define BZ_MATCH_MAX_GAMES (1 << 24)
/* error word: 0, or the kind and the slot of the FIRST refused move (sticky; the slot is frozen as it stood, every
 * other game goes on): the side to move handed in an action that is not a legal move / no action at all (-1) */
#define BZ_MATCH_ERR_ILLEGAL 0xC0000000u
#define BZ_MATCH_ERR_NO_ACTION 0xA0000000u
#define BZ_MATCH_ERR_SLOT_MASK 0x00FFFFFFu
/* offsets (bytes, from the workspace base) of the caller-visible arrays */
typedef struct bz_match_layout {
    int64_t own, opp;               /* u64 [B] position seen by the side to move = the roots of both engines */
    int64_t to_move;                /* i8 [B] absolute colour of the side to move */
    int64_t active;                 /* u8 [B] 1 = running, 0 = finished, 2 = frozen by a refused move */
    int64_t winner;                 /* i8 [B] absolute colour +1 / -1 / 0, valid once the slot has finished */
    int64_t plies;                  /* i32 [B] moves made */
    int64_t a_colour;               /* i8 [B] the colour side A plays */
    int64_t to_move_a, to_move_b;   /* i8 [B] to_move of the next search's roots per engine: the colour where that side is
                                     * to move in a running slot past its opening, else 0 (slot idle in that engine) */
    int64_t log_action, log_mover;  /* u8 / i8 [max_plies][B]: 255 / 0 = no move by this slot at this ply */
    int32_t n_games, max_plies;
} bz_match_layout;
/* what the host reads once per ply: the state BEFORE ply `ply` (the next one to be played) */
typedef struct bz_match_hdr {
    int32_t ply;                    /* plies played so far */
    int32_t n_active;               /* running slots */
    int32_t n_to_move_a, n_to_move_b; /* slots the next search of engine A / B serves (0: that engine need not search) */
    uint32_t error;                 /* BZ_MATCH_ERR_* | slot, or 0 */
    uint32_t engine_err_a, engine_err_b; /* the BZ_ENGINE_ERR_* bits the engines raised in any search so far */
    uint32_t reserved;
} bz_match_hdr;
/* game: BZ_GAME_*; n_games even, 2 .. BZ_MATCH_MAX_GAMES; max_plies 1..64 rows of the move log, 0 = the game's longest
 * game (9 / 60 / 32 / 12).  Needs no GPU; -1 (bz_last_error says why) for bad arguments. */
int64_t bz_match_workspace_bytes(int32_t game, int32_t n_games, int32_t max_plies);
/* workspace: device memory of >= bz_match_workspace_bytes bytes, 256-byte aligned, owned by the caller */
int32_t bz_match_create(int32_t game, int32_t n_games, int32_t max_plies, void* workspace, int64_t workspace_bytes,
                        bz_match** out);
int32_t bz_match_destroy(bz_match* m);
int32_t bz_match_get_layout(const bz_match* m, bz_match_layout* out);
/* every slot at the game's start position (any board size), colours, an empty log, the roots of ply 0 */
int32_t bz_match_begin(bz_match* m, uint64_t seed, int32_t opening_plies, void* stream);
/* one ply of every running slot.  action_a / action_b: device i32 [B] as bz_engine_root_policy writes them (-1 = idle);
 * the action of the side to move is played (the opening move during a slot's opening).  engine_a / engine_b (optional,
 * may be null): the engines, whose error words the kernel folds into the header.  A refused move is reported through
 * the header's error word, never through a fault.  BZ_ESTATE after max_plies plies. */
int32_t bz_match_ply(bz_match* m, const int32_t* action_a, const int32_t* action_b, const bz_engine* engine_a,
                     const bz_engine* engine_b, void* stream);
/* synchronises the stream: the ONE host read of a ply */
int32_t bz_match_header(bz_match* m, void* stream, bz_match_hdr* out);
/* the opening draw, host side: *index = rng_draw(seed ^ C_MATCH, pair, ply) mod n_legal (1 <= n_legal <= 64) */
int32_t bz_match_opening_index(uint64_t seed, uint64_t pair, int32_t ply, int32_t n_legal, int32_t* index);
/* one search for n engines (n <= 16), engine i on streams[i], issued by ONE host thread and interleaved tree step by
 * tree step like bz_engines_step, without the play: each engine with its own simulations, leaves per step and mode
 * (an engine whose search is one fused launch is simply launched).  engines[i] may be null (skipped).  Results are
 * those of bz_engine_search on every engine.  run_ahead_sims as in bz_engines_step. */
int32_t bz_engines_search(bz_engine* const* engines, void* const* streams, int32_t n, int32_t run_ahead_sims);

/* ------------------------------------------------------------------------ */
/* Training step of the residual tower: hand-written  */
/* bf16 MFMA kernels for forward-with-saved-activations, backward-data and   */
/* backward-weights of its n_layers = 2 NB conv3x3 layers.  The loop they    */
/* serve has the shape of src/tic_tac_toe/SL/train.py:85-136 (forward, loss, */
/* backward, Adam step); stem, heads, losses and the optimiser are the next   */
/* section's entry points (or the caller's own); the fp32 master weights stay */
/* with the caller.  C = 64 or 128.                                           */
/*                                                                           */
/* Tensors (device, bf16 unless noted), n = batch (a multiple of             */
/* bz_train_positions_per_workgroup(C)):                                     */
/*   act[a], a = 0..L : [n][64 cells][C]  act[0] = the stem's output (after   */
/*                      its ReLU), act[a] = output of conv layer a - 1        */
/*   g[a],   a = 0..L : [n][64][C]  g[a] = d loss / d (pre-activation of      */
/*                      act[a]) for a >= 1; g[0] = d loss / d act[0]          */
/*   W (fp32)         : [L][C co][C ci][3][3]  torch Conv2d layout, stacked   */
/*   wf_fwd / wf_bwd  : bz_train_wf_bytes() each: the kernels' fragment-major */
/*                      weight streams (bz_train_pack_weights writes both)    */
/*   masks            : bz_train_mask_bytes(): the ReLU pattern of act[1..L]  */
/* ------------------------------------------------------------------------ */
int64_t bz_train_wf_bytes(int32_t C, int32_t n_layers);
int32_t bz_train_positions_per_workgroup(int32_t C);
int64_t bz_train_mask_bytes(int32_t C, int32_t n_layers, int32_t n);
int32_t bz_train_pack_weights(const float* W, int32_t C, int32_t n_layers, void* wf_fwd, void* wf_bwd, void* stream);
/* act0 = act[0]; acts_out = act[1..L] as [L][n][64][C]; bias fp32 [L][C] */
int32_t bz_train_tower_fwd(const void* act0, const void* wf_fwd, const float* bias, int32_t C, int32_t n_layers, int32_t n,
                           void* acts_out, void* masks, void* stream);
/* g_top = g[L]; gs_out = g[0..L-1] as [L][n][64][C]; zeros_c = C fp32 zeros */
int32_t bz_train_tower_bwd(const void* g_top, const void* wf_bwd, const float* zeros_c, const void* masks, int32_t C,
                           int32_t n_layers, int32_t n, void* gs_out, void* stream);
/* weight gradients: acts = act[0..L-1], gs = g[1..L], both [L][n][64][C].  partial (fp32) =
 * [L][splits][9 taps][C ci][C co] and db_partial (fp32) = [L][bz_train_wgrad_bias_rows(C, splits)][C]: the caller sums over
 * the second axis of both (bz_train_wgrad_splits()) and permutes the former to W's layout; the latter is the bias gradient
 * (sum of g[l + 1] over positions and cells).  (bz_train_finish does both.) */
int32_t bz_train_wgrad_splits(int32_t C, int32_t n_layers, int32_t n);
int32_t bz_train_wgrad_bias_rows(int32_t C, int32_t splits);
int32_t bz_train_wgrad(const void* acts, const void* gs, int32_t C, int32_t n_layers, int32_t n, int32_t splits, float* partial,
                       float* db_partial, void* stream);

/* ------------------------------------------------------------------------ */
/* The two ends of the same step (csrc/bz_train_ends.hip), so that a whole   */
/* step -- train.py:85-136's forward, loss, backward -- is 9 launches        */
/* (10 with the optimiser):                                                   */
/*   stem_fwd, pack_weights, tower_fwd, heads, tower_bwd, wgrad, stem_wgrad, */
/*   heads_wgrad, finish (+ the Adam update as a tenth launch).  The net is     */
/* (bz_train_optim_step, the extended optimiser: two launches in its place.)  */
/* betazero_amd/net.py's (SURVEY 8(d) "net"): every pointer below is one of   */
/* its parameter tensors (fp32, torch layout) or the gradient of one.         */
/* n = batch, a multiple of 4 (and of bz_train_positions_per_workgroup(C)).   */
/* ------------------------------------------------------------------------ */
typedef struct bz_train_head_params {   /* pol: Conv2d(C, 2, 1); polfc: Linear(128, 65); val: Conv2d(C, 1, 1); v1: Linear(64, VH); v2: Linear(VH, 1) */
    const float *pol_w, *pol_b, *polfc_w, *polfc_b, *val_w, *val_b, *v1_w, *v1_b, *v2_w, *v2_b;
} bz_train_head_params;
typedef struct bz_train_tensors {       /* one fp32 device pointer per parameter tensor of the net: the gradients, the parameters, an Adam moment */
    float *stem_w, *stem_b, *tower_w, *tower_b, *pol_w, *pol_b, *polfc_w, *polfc_b, *val_w, *val_b, *v1_w, *v1_b, *v2_w, *v2_b;
} bz_train_tensors;
typedef struct bz_train_partials {      /* the partial sums the kernels of one step leave behind */
    const float *tower, *tower_b;       /* bz_train_wgrad's partial / db_partial */
    const float *stem, *heads, *heads_w; /* bz_train_stem_wgrad's, bz_train_heads', bz_train_heads_wgrad's (bz_train_ends_sizes) */
    int32_t splits;                     /* bz_train_wgrad's splits */
} bz_train_partials;
/* The batch of a step.  This struct lives in DEVICE memory and is read by the kernels at launch time: a step captured
 * into a HIP graph keeps working when the data set's tensors are replaced or another batch is drawn -- the host rewrites
 * these 48 bytes (or just the idx array).  Batch position p is row idx[p] of the data set, or row p when idx is NULL.  An
 * index outside [0, n_rows) never becomes a fault -- the kernels read row 0 / n_rows - 1 in its place -- but it is an ERROR:
 * every such batch position is counted into the step's error word, losses[3] of bz_train_finish (the reference's
 * index_select-style gather, SL/train.py:102-108, raises on it).  The rows are what bz_engine_pack_examples / the example block hold: (s, pi, z) of
 * generate_training_games.py:12-23 in own/opp form. */
typedef struct bz_train_batch {
    const uint64_t *own, *opp;          /* [n_rows] bitboards, side-to-move canonical */
    const float* pi;                    /* [n_rows][65] */
    const int8_t* z;                    /* [n_rows] */
    const int64_t* idx;                 /* [n] or NULL */
    int64_t n_rows;
} bz_train_batch;
/* Adam behind bz_train_finish (torch.optim.Adam's arithmetic without weight decay / amsgrad: what train.py:87 constructs):
 * one more launch that updates all 14 parameter tensors from the gradients just written.  hyper = 16 bytes of DEVICE memory
 * {float learning rate; float steps done so far; float warm-up steps; float unused}: bz_train_finish advances the step
 * count to t = steps done + 1 and the update runs at rate lr * min(1, t / warm-up) (warm-up 0: lr), so a captured graph can
 * be replayed step after step with no host write in between; the caller writes the block to (re)start or change the rate. */
typedef struct bz_train_adam {
    float* hyper;
    float beta1, beta2, eps;
    bz_train_tensors p, m, v;           /* parameters (updated in place), first and second moments (zero before step 1) */
} bz_train_adam;
/* sizes[0..5] = number of partial vectors, floats per vector of: stem_wgrad, heads, heads_wgrad */
int32_t bz_train_ends_sizes(int32_t C, int32_t n, int32_t* sizes);
/* act0[pos][cell][c] (bf16) = relu(conv3x3(planes(own, opp)))[c][cell]: the bit planes never exist in memory */
int32_t bz_train_stem_fwd(const bz_train_batch* batch_dev, int32_t n, const float* stem_w, const float* stem_b, int32_t C, void* act0,
                          void* stream);
/* g0 = g[0] (d loss / d act[0], what bz_train_tower_bwd leaves there); partial [sizes[0]][sizes[1]] */
int32_t bz_train_stem_wgrad(const bz_train_batch* batch_dev, const void* act0, const void* g0, int32_t n, int32_t C, float* partial,
                            void* stream);
/* heads + losses, forward and backward: act_top = act[L]; loss = mean CE(pi, softmax(logits)) + mean (v - z)^2 over the
 * batch.  Writes g_top = g[L] (bf16 [n][64][C], the input of bz_train_tower_bwd), the per-position operands of the FC
 * weight gradients (hv fp32 [n][192], dl [n][65], dv1 [n][64]) and partial [sizes[2]][sizes[3]]. */
int32_t bz_train_heads(const void* act_top, const bz_train_batch* batch_dev, int32_t n, int32_t C, int32_t VH,
                       const bz_train_head_params* P, void* g_top, float* hv, float* dl, float* dv1, float* partial, void* stream);
/* The same with a float value target: loss = mean CE + mean (v - vt)^2.  vt_slot_dev is ONE pointer-sized word
 * in DEVICE memory holding the address of an fp32 [n_rows] array, gathered by the batch's idx with the same clamping and
 * error word as z -- a device word for the reason bz_train_batch lives in device memory: a captured step keeps working when
 * the data set (and its targets) is replaced.  Everything else is bz_train_heads: with vt == (float)z every output is the
 * same bits. */
int32_t bz_train_heads_vt(const void* act_top, const bz_train_batch* batch_dev, const float* const* vt_slot_dev, int32_t n,
                          int32_t C, int32_t VH, const bz_train_head_params* P, void* g_top, float* hv, float* dl, float* dv1,
                          float* partial, void* stream);
/* The ownership head in the step (KataGo, Wu 2019, section 5): a fourth 1x1 plane on act[L], Conv2d(C, 1, 1)
 * with a tanh, trained on every row's ownership target.  Its C + 1 parameters belong to no bz_train_tensors:
 * the net the engine plays with does not have them.  Per position, lane = cell, fp32 on the bf16 act[L]:
 *   d3 = ob + sum_c x[cell][c] ow[c]  (one fmaf chain, c ascending);  o = tanhf(d3);  t = bit_cell(fown[row]) - bit_cell(fopp[row])
 *   L_own = mean over positions and all 64 cells of (o - t)^2;  dp3 = own_weight * 2 (o - t)(1 - o^2) * (1 / n) / 64
 * dp3 joins bz_train_heads' backward: d ob += dp3, d ow[c] += sum_cell dp3 x, and g_top gains fmaf(dp3, ow[c], .) as its LAST
 * term -- with weight = 0 every output of bz_train_heads keeps its value.  The rows are gathered by the batch's idx, with the
 * same clamping and the same error word. */
typedef struct bz_train_own {
    const float *w, *b;                /* the head's parameters: weight [C], bias [1] (device) */
    const uint64_t* const* targets;    /* DEVICE slot of two pointers: fown [rows], fopp [rows] -- a device slot for the reason
                                          vt_slot_dev is one: a captured step survives a new data set */
    float weight;                      /* own_weight: finite, >= 0 */
    float* partial;                    /* [sizes[2]][C + 2] (bz_train_ends_sizes): per workgroup d ow [C], d ob, L_own */
} bz_train_own;
/* bz_train_heads / bz_train_heads_vt with the ownership head (k_train_heads_own / k_train_heads_own_vt): every output of
 * theirs, plus own->partial */
int32_t bz_train_heads_own(const void* act_top, const bz_train_batch* batch_dev, const bz_train_own* own, int32_t n, int32_t C,
                           int32_t VH, const bz_train_head_params* P, void* g_top, float* hv, float* dl, float* dv1, float* partial,
                           void* stream);
int32_t bz_train_heads_own_vt(const void* act_top, const bz_train_batch* batch_dev, const float* const* vt_slot_dev,
                              const bz_train_own* own, int32_t n, int32_t C, int32_t VH, const bz_train_head_params* P, void* g_top,
                              float* hv, float* dl, float* dv1, float* partial, void* stream);
/* The head's own end of the step, one launch of one workgroup behind bz_train_finish (and bz_train_optim_step), which have
 * advanced the step counter: own->partial summed in a fixed order (no atomics, no memset) -> grad_w [C], grad_b [1],
 * own_loss[0] = L_own; losses (may be null) [0] += own_weight * L_own -- bz_train_finish stored CE + MSE there in this step.
 * opt (may be null): plain Adam (bz_train_finish's arithmetic) on the C + 1 parameters, with the rate, the step number and the
 * warm-up of `hyper` = the step's optimiser's hyper block; when one of the C + 1 gradients is not finite, parameters and
 * moments stay as they are.  Under the extended optimiser the head's parameters are outside its norm, decay and EMA (the engine
 * never reads them); their gradient's way into the trunk, g_top, is inside. */
typedef struct bz_train_own_adam {
    const float* hyper;
    float beta1, beta2, eps;
    float *pw, *pb, *mw, *mb, *vw, *vb;   /* parameters and the two Adam moments: weight [C], bias [1] */
} bz_train_own_adam;
int32_t bz_train_own_finish(const bz_train_own* own, int32_t C, int32_t n, float* grad_w, float* grad_b, float* own_loss, float* losses,
                            const bz_train_own_adam* opt, void* stream);
/* partial [sizes[4]][sizes[5]] */
int32_t bz_train_heads_wgrad(const float* hv, const float* dl, const float* dv1, int32_t n, int32_t VH, float* partial, void* stream);
/* every partial sum -> the gradient tensors G (torch layouts); losses[4] = loss, policy CE, value MSE of the batch, and the
 * ERROR WORD: losses[3] += the number of batch positions of this step whose row index was out of range (bz_train_batch).
 * The error word accumulates over steps (a graph can be replayed many times before the host looks): the caller zeroes it,
 * and a value != 0 when the losses are read means some step trained on a wrong row.
 * opt != NULL: followed by the Adam update of every parameter (a second launch) */
int32_t bz_train_finish(const bz_train_partials* Q, const bz_train_tensors* G, int32_t C, int32_t n_layers, int32_t VH, int32_t n,
                        float* losses, const bz_train_adam* opt, void* stream);
/* The extended optimiser: AdamW with decoupled weight decay (torch.optim.AdamW's arithmetic, two parameter groups), a clip of
 * the GLOBAL gradient norm (torch.nn.utils.clip_grad_norm_'s rule), a refusal of non-finite steps and an exponential moving
 * average of the parameters.  Called AFTER bz_train_finish(..., opt = NULL, ...) on the gradients G it left: two more launches
 * (k_train_gnorm, k_train_optim), so the extended step is eleven.  With weight decay 0, max norm 0, no EMA tensors and finite
 * gradients the update is bit for bit the one of bz_train_finish(..., opt != NULL).
 *   hyper: 32 bytes of DEVICE memory {lr; steps ATTEMPTED so far t; warm-up steps; weight decay; max norm (0: no clip); EMA
 *     decay d; 0; 0}, read at launch time (a captured graph follows a host write).  bz_train_optim_hyper lays the block out in
 *     host memory and refuses (BZ_EINVAL) a negative or non-finite lr / t / warm-up / weight decay / max norm and an EMA decay
 *     outside [0, 1); the caller copies it to the device.  k_train_gnorm advances t by one, whether or not the update follows.
 *   norm = sqrtf(sum of g^2 over all 14 tensors), a fixed-order fp32 sum with no atomics and no zeroed buffer;
 *     partials: bz_train_optim_partials() floats of DEVICE scratch, every one rewritten by every step.
 *   skip  = !(norm < +inf): a NaN or an infinity anywhere among the gradients, or a square that overflowed (|g| > 1.8e19):
 *     NOTHING of p, m, v, ema is written by that step (t has advanced all the same).
 *   scale = max norm > 0 ? fminf(1, max norm / (norm + 1e-6f)) : 1;   g' = g * scale;   lr_t, bc1, bc2_rsqrt as in bz_train_adam
 *   m' = fmaf(beta1, m, (1 - beta1) g');  v' = fmaf(beta2, v, (1 - beta2) g' g')
 *   p' = p * (1 - lr_t * wd_j) - (lr_t / bc1) * m' / (sqrtf(v') * bc2_rsqrt + eps)
 *     wd_j = the weight decay for the seven *_w tensors, and for the seven *_b tensors only with decay_biases != 0 (else 0)
 *   ema' = fmaf(1 - d, p' - ema, ema)   (only with ema != NULL; the caller starts ema at a copy of p)
 *   stats: 16 bytes of DEVICE memory {norm of the last step before the clip; scale it applied (0: skipped); steps skipped;
 *     steps clipped (scale < 1)}: the two counts accumulate until the caller zeroes them, like losses[3]. */
typedef struct bz_train_optim {
    float* hyper;
    float* stats;
    float* partials;
    float beta1, beta2, eps;
    int32_t decay_biases;
    bz_train_tensors p, m, v;           /* as in bz_train_adam */
    const bz_train_tensors* ema;        /* the averaged parameters (updated in place), or NULL */
} bz_train_optim;
int32_t bz_train_optim_partials(void);
int32_t bz_train_optim_hyper(float lr, float steps_done, float warmup_steps, float weight_decay, float max_norm, float ema_decay,
                             float* block8_host);
/* BZ_EINVAL (with a message) for a null pointer in G / opt (ema alone may be NULL), betas outside [0, 1), eps <= 0, C other than
 * 64 / 128, n_layers < 2 or VH outside 1..64; BZ_ENOGPU without a device */
int32_t bz_train_optim_step(const bz_train_tensors* G, const bz_train_optim* opt, int32_t C, int32_t n_layers, int32_t VH, void* stream);

/* ------------------------------------------------------------------------ */
/* fp8 quantisation-aware training: the step's forward is the */
/* fp8 net's (bz_net_forward_fp8), run on the bf16 MFMA training tower with   */
/* exact operands; the backward is the straight-through estimator.  The rule  */
/* (csrc/bz_qat.h; betazero_amd/quant.py):                                    */
/*   weights     : w_b = bf16_RNE(w); m = max |w_b| over the output channel   */
/*                 (a NaN is skipped); s = 2^floor(log2(448 / m)), 1 for m = 0;*/
/*                 w_q = e4m3_RNE_sat(w_b s) / s (a NaN weight stays a NaN)     */
/*   activations : a = e4m3_RNE_sat(16 maximum(v, +0)) / 16 from the fp32 value */
/*                 (one rounding; a NaN passes, +inf becomes 28)               */
/* Offered where the fp8 tower exists: C == 128, anything else is BZ_EINVAL.  */
/* ------------------------------------------------------------------------ */
/* host: one output channel (n = C 9 for a tower channel, C for a head row); scale may be NULL */
int32_t bz_qat_weight_row(const float* w, int32_t n, float* w_q, float* scale);
/* host: the stored activation of the fp32 value v */
float bz_qat_act(float v);
/* device: the kernels' form of bz_qat_act (the fp8 conversion instructions) over n floats in device memory */
int32_t bz_qat_act_batch(const float* in, float* out, int64_t n, void* stream);
/* k_qat_scales: scales [n_layers C + 3] = the tower's per-output-channel scales, then those of the 3 head conv1x1 rows (pol.weight
 * [2][C], val.weight [C]); head_q [3][C] = those rows fake-quantised (what bz_train_head_params.pol_w / val_w point at in a QAT
 * step: the gradients still go to the masters) */
int32_t bz_train_qat_scales(const float* W, const float* pol_w, const float* val_w, int32_t C, int32_t n_layers, float* scales,
                            float* head_q, void* stream);
/* k_qat_pack: bz_train_pack_weights' two streams with w_q in every entry (backward-data sees the quantised weights too) */
int32_t bz_train_qat_pack_weights(const float* W, const float* scales, int32_t C, int32_t n_layers, void* wf_fwd, void* wf_bwd,
                                  void* stream);
/* k_qat_fwd / k_qat_stem: bz_train_tower_fwd / bz_train_stem_fwd with the activation rule on every stored activation; the ReLU
 * masks are those of the STORED values (a positive value that rounds to 0 passes no gradient; saturation at 28 is not masked) */
int32_t bz_train_qat_tower_fwd(const void* act0, const void* wf_fwd, const float* bias, int32_t C, int32_t n_layers, int32_t n,
                               void* acts_out, void* masks, void* stream);
int32_t bz_train_qat_stem_fwd(const bz_train_batch* batch_dev, int32_t n, const float* stem_w, const float* stem_b, int32_t C, void* act0,
                              void* stream);

/* ------------------------------------------------------------------------ */
/* A board symmetry per row inside the training step (the     */
/* per-position rotation / reflection of AlphaGo Zero's minibatches): batch   */
/* position p trains on row idx[p] of the data set under the element sym[p]   */
/* of the evaluation symmetries above (0..6 = bz_augment_d4_batch's           */
/* transforms 0..6, 7 = the anti-transpose).  ONE staging kernel in front of  */
/* the stem, k_train_sym_batch, writes the n transformed rows into a staging  */
/* batch; the step's own bz_train_batch points at that batch with idx = NULL, */
/* its vt slot and its ownership slot at the staged columns, and every other  */
/* kernel of the step runs as it is.  Per row (csrc/bz_train_sym.h):          */
/*   own, opp, fown, fopp -> T_s on the size x size corner (bz_sym_board)     */
/*   pi'[tau_s(j)] = pi[j]; the pass entry 64 and cells outside the corner    */
/*     stay; the 65 entries are moved as 32-bit patterns                      */
/*   z, vt copied                                                             */
/* ------------------------------------------------------------------------ */
/* the data set's optional columns and the batch's symmetries: DEVICE memory, read at launch time like bz_train_batch and
 * for the same reason (a captured step survives a new data set) */
typedef struct bz_train_sym_cols {
    const float* vt;                    /* [n_rows] or NULL */
    const uint64_t *fown, *fopp;        /* [n_rows] or NULL */
    const uint8_t* sym;                 /* [n]: the symmetry of batch position p */
} bz_train_sym_cols;
/* the staging batch (host struct of device pointers, all [n]; pi [n][65]); vt, and fown / fopp together, may be NULL */
typedef struct bz_train_sym_stage {
    uint64_t *own, *opp;
    float* pi;
    int8_t* z;
    float* vt;
    uint64_t *fown, *fopp;
} bz_train_sym_stage;
/* rows a workgroup of k_train_sym_batch stages (64): bad_dev below holds ceil(n / this) words */
int32_t bz_train_sym_rows_per_workgroup(void);
/* src_dev: the data set and the batch's idx (idx NULL: rows 0..n-1); n: 1 .. 2^24; size: 1..8.  An index outside [0, n_rows) is
 * clamped as bz_train_batch says, a symmetry outside 0..7 is taken & 7; either is an ERROR of the caller that the staged
 * step can no longer see: each such batch position is ADDED to its workgroup's word of bad_dev (uint32 per workgroup, owned by
 * that workgroup alone: no atomics, no memset), which the caller sums into the step's error word and zeroes with it.  A
 * staged optional column whose source address is NULL is left as it is. */
int32_t bz_train_sym_batch(const bz_train_batch* src_dev, const bz_train_sym_cols* cols_dev, int32_t n, int32_t size,
                           const bz_train_sym_stage* stage, uint32_t* bad_dev, void* stream);
/* host: one row through the code the kernel runs.  s 0..7, size 1..8; pi / pi_out [65], distinct; fown_out / fopp_out may be
 * NULL */
int32_t bz_train_sym_row(uint64_t own, uint64_t opp, const float* pi, uint64_t fown, uint64_t fopp, int32_t size, int32_t s,
                         uint64_t* own_out, uint64_t* opp_out, float* pi_out, uint64_t* fown_out, uint64_t* fopp_out);

/* ------------------------------------------------------------------------ */
/* In-library kernel timers: HIP events recorded on the launch stream around  */
/* each launch of the named kernel (off by default; bench.py turns them on).  */
/* ------------------------------------------------------------------------ */
enum { BZ_PROF_TOWER = 0, BZ_PROF_STEM = 1, BZ_PROF_HEADS = 2, BZ_PROF_SELECT = 3, BZ_PROF_EXPAND_BACKUP = 4,
       BZ_PROF_SEARCH_FUSED = 5, BZ_PROF_PLAY = 6, BZ_PROF_ENV_STEP = 7, BZ_PROF_N = 8 };
int32_t bz_profile_enable(int32_t on);
/* create the events for n_launches launches of a slot up front (keeps event creation out of a
 * timed loop); a slot records at most 262,144 launches between two resets */
int32_t bz_profile_reserve(int32_t slot, int64_t n_launches);
/* synchronises the device; launches = all launches seen, timed = launches that
 * carried events (capped), total_ms = sum of their durations */
int32_t bz_profile_read(int32_t slot, int64_t* launches, int64_t* timed, double* total_ms);
int32_t bz_profile_reset(void);
/* start/end (ms, relative to the slot's first event) of every timed launch; launches issued on
 * different streams may overlap in time */
int32_t bz_profile_intervals(int32_t slot, double* starts_ms, double* ends_ms, int64_t cap, int64_t* n);

/* Do two HIP streams run side by side?  Starts one single-wave kernel that waits spin_us microseconds on each of
 * them behind a common event and reports max(completion time) / spin_us, best of `reps`: ~1.0 = the streams
 * overlap, ~2.0 = the second waited for the first (e.g. they share a hardware queue).  The pipelined self-play
 * (two engines on two streams) picks its stream pair with it.  Synchronises both streams. */
int32_t bz_stream_overlap_probe(void* stream_a, void* stream_b, int32_t spin_us, int32_t reps, float* serial_ratio);

/* ------------------------------------------------------------------------ */
/* The float primitives of csrc/bz_math.h one at a time, as   */
/* the host build or as the gfx950 build of one translation unit computes     */
/* them: what the tests compare the two builds through.                       */
/* ------------------------------------------------------------------------ */
enum { BZ_PROBE_EXPF = 0, BZ_PROBE_LOGF = 1, BZ_PROBE_TANHF = 2, BZ_PROBE_FSQRT = 3, BZ_PROBE_FDIV = 4, BZ_PROBE_U01 = 5,
       BZ_PROBE_HASH_LOGIT = 6, BZ_PROBE_HASH_VALUE = 7, BZ_PROBE_GAMMA = 8 };
enum { BZ_PROBE_HOST = 0, BZ_PROBE_DEVICE = 1 };
enum { BZ_PROBE_MAP = 0, BZ_PROBE_SWEEP = 1 };
/* where = BZ_PROBE_HOST: a, b, out are host pointers, stream is ignored and HIP is never touched (runs without a GPU).
 * where = BZ_PROBE_DEVICE: device pointers, the work is queued on `stream`.
 * mode = BZ_PROBE_MAP: out[i] (float [n], the result's bits untouched) = op of element i.  Operands:
 *   EXPF, LOGF, TANHF, FSQRT  a = float [n]
 *   FDIV                      a / b, both float [n]
 *   U01, HASH_VALUE           a = uint64 [n]
 *   HASH_LOGIT                a = uint64 [n] (the position hash), b = uint64 [n] (the action)
 *   GAMMA                     a = float [n] (alpha), b = uint64 [n][4] (seed, game, ply, edge)
 * mode = BZ_PROBE_SWEEP (EXPF, LOGF, TANHF, FSQRT): the op at every 32-bit pattern p in [lo, hi), hi <= 2^32; a, b, n are
 *   ignored.  out = uint64 [((hi - 1) >> 24) - (lo >> 24) + 1], one checksum per chunk of 2^24 patterns:
 *   out[(p >> 24) - (lo >> 24)] = sum over the chunk's p of mix64(p << 32 | canon(bits of op(p))) mod 2^64, where canon
 *   turns every NaN into 0x7FC00000.  The sum does not depend on the order: host and device give the same number exactly
 *   when they agree on every pattern of the chunk (up to a 2^-64 coincidence). */
int32_t bz_spec_probe(int32_t op, int32_t where, int32_t mode, const void* a, const void* b, int64_t n, uint64_t lo, uint64_t hi,
                      void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BZ_ABI_H */
