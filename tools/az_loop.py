#!/usr/bin/env python3
"""The closed AlphaZero loop on one GPU, end to end through the package's public pieces:

    self-play (PipelinedSelfPlay: two engines on two streams, bf16 MFMA net in the loop, Dirichlet root noise, temperature moves)
      -> example block -> 80 / 20 hold-out split of the new rows (the reference's split, SL/train.py:66-78)
      -> 8-fold D4 augmentation + exact dedupe of the training part on the device (augment_examples)
      -> with --reanalyse-frac F: reanalysis of the older window slots (Reanalyser): a seeded share F of every
         older slot's un-augmented training rows is searched again with the net self-play just used and gets that search's pi
         (and kl); the slot is augmented again
      -> with --merge-positions: position averaging of the training window (merge_positions): the rows of one
         position become one row with the mean pi and the mean value target
      -> with --train-symmetry: no augmentation at all: the window holds the rows as they were played and every
         step draws a board symmetry per batch position, applied by a staging kernel inside the fused step
      -> policy cross-entropy + value MSE steps on the hand-written training kernels replayed as one HIP graph
         (GraphedTrainStep: stem, tower, heads, losses, every gradient and Adam as ten launches; --miopen-train /
         --eager-train / --fp32-train fall back to stock PyTorch autograd, run eagerly)
         -- the rows never leave the GPU between the engine's example block and the optimiser step
      -> validation on the held-out rows with the engine's own bf16 MFMA forward (validate: policy CE, value MSE, top-1
         agreement -- the reference's per-epoch validation line, SL/train.py:121-146)
      -> weights pushed back into the engine's net (refresh_device_net)
      -> with --fp8: all of the above with the fp8 net in the loop (net_fp8 self-play, gate and arena; 128 channels) and the
         training step quantisation-aware (fp8_qat: the fp8 net's forward, straight-through gradients -- DESIGN.md 12.3);
         --fp8-no-qat keeps the plain bf16 step as the ablation.  The validation line is then the fp8 forward's too
      -> batched arena against the reference's depth-limited minimax player (play_arena)
      -> with --gate-games N: a head-to-head match (play_match) of the freshly trained net against the net
         self-play currently uses; the candidate is promoted to self-play only at score >= --gate-score (AlphaGo Zero's
         0.55), otherwise self-play keeps the old weights while training continues from the new ones

It prints one JSON line per iteration and a final summary; `--out` keeps them.  The yard-stick is the reference's
OptimalPlayer (src/reversi/players/reversi_players.py:35-77, stone-difference minimax) at `--depth`; the same arena
with the uniform evaluator (no net) is printed first as the untrained reference point.

    python tools/az_loop.py --iters 8            # a few minutes on one MI355X
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betazero_amd.arena import play_arena  # noqa: E402
from betazero_amd.augment import augment_examples  # noqa: E402
from betazero_amd.engine import (EvalSymmetry, ForcedPlayouts, Fpu, GumbelConfig, PipelinedSelfPlay, PlayoutCap, Resign, check_forced_playouts,  # noqa: E402
                                 check_early_stop, check_fpu, check_playout_cap, check_resign, check_solver, concat_device_examples)
from betazero_amd.merge import merge_positions, merged_repeats  # noqa: E402
from betazero_amd.match import MatchPlayer, play_match  # noqa: E402
from betazero_amd.reanalyse import Reanalyser, reanalyse_rows  # noqa: E402
from betazero_amd.net import DeviceNet, OwnershipHead, PolicyValueNet  # noqa: E402
from betazero_amd.surprise import surprise_resample  # noqa: E402
from betazero_amd.value_targets import value_targets  # noqa: E402
from betazero_amd.train import (GraphedTrainStep, holdout_split, make_optimizer, refresh_device_net, select_rows,  # noqa: E402
                                train_step, validate)


# how --resign-threshold moves between iterations (untuned): down fast when resignations turn out wrong, up slowly when they are safe
RESIGN_STEP_DOWN, RESIGN_STEP_UP, RESIGN_T_MIN, RESIGN_T_MAX = 0.05, 0.01, -0.99, -0.5


def next_resign_threshold(threshold, stats, fp_target):
    """the threshold of the next iteration from this one's resign_stats()"""
    rate = stats["false_positive_rate"]
    if rate is None:  # no played-out game would have resigned: nothing was measured
        return threshold
    if rate > fp_target:
        threshold -= RESIGN_STEP_DOWN
    elif rate < fp_target / 2:
        threshold += RESIGN_STEP_UP
    return min(max(threshold, RESIGN_T_MIN), RESIGN_T_MAX)


# the arguments a resumed run may change: everything else shapes the state or the run's course and must be the checkpoint's
RESUME_FREE = ("iters", "checkpoint", "checkpoint_every", "no_checkpoint_window", "resume", "init_net", "out", "save_net")


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64, choices=(64, 128, 256))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--games", type=int, default=2048, help="concurrent self-play games per iteration")
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--pipelines", type=int, default=2, help="self-play pipelines on separate HIP streams (PipelinedSelfPlay)")
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--window", type=int, default=3, help="iterations of examples kept for training")
    ap.add_argument("--epochs", type=float, default=1.0, help="passes over the (augmented) window per iteration")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--lr-warmup", type=int, default=300, help="steps over which the learning rate ramps up (GraphedTrainStep.lr_warmup_steps): "
                    "without it Adam's first steps at this lr can kill the head ReLUs -- profiles/r04_channels_last_cause.txt")
    ap.add_argument("--val-split", type=float, default=0.2, help="fraction of every iteration's rows held out for validation "
                    "(the reference's validation_split, SL/train.py:66); 0 = train on everything")
    ap.add_argument("--temp-moves", type=int, default=10)
    ap.add_argument("--arena-games", type=int, default=256)
    ap.add_argument("--arena-sims", type=int, default=64)
    ap.add_argument("--depth", type=int, default=3, help="search depth of the minimax opponent")
    ap.add_argument("--final-depths", default="1,3,5", help="minimax depths the final net is also played against")
    ap.add_argument("--opening-plies", type=int, default=4, help="random legal moves before the arena players take over")
    ap.add_argument("--gumbel", action="store_true", help="self-play with Gumbel root search (DESIGN.md 3.13): the example rows' pi is the "
                    "improved policy, Gumbel noise on the first --temp-moves moves, no Dirichlet noise; the gate's and the arena's players "
                    "then play the Gumbel move too")
    ap.add_argument("--gumbel-interior", action="store_true", help="under --gumbel: the Gumbel interior rule below the root (DESIGN.md "
                    "3.21; the action whose visit share lags the node's improved policy the most) instead of PUCT, in self-play, for "
                    "both players of the gate and for the arena's search player.  An argument error without --gumbel")
    ap.add_argument("--fast-sims", type=int, default=0, help="self-play with playout cap randomisation (DESIGN.md 3.15): every move "
                    "is searched with --sims simulations with probability --full-prob (and recorded) or with this many (and not "
                    "recorded); 0 = off.  Not with --gumbel")
    ap.add_argument("--full-prob", type=float, default=0.25, help="probability of a full search under --fast-sims")
    ap.add_argument("--forced-k", type=float, default=0.0, help="self-play with forced playouts and policy target pruning (DESIGN.md "
                    "3.16; KataGo uses 2): every visited root child is searched up to sqrt(k P sum N) visits and the recorded pi drops "
                    "the visits PUCT would not have made; 0 = off.  Composes with --fast-sims (full searches only) and the Dirichlet "
                    "noise; not with --gumbel")
    ap.add_argument("--no-prune", action="store_true", help="under --forced-k: record the raw N / sum N (ablation)")
    ap.add_argument("--surprise", action="store_true", help="policy surprise weighting (DESIGN.md 3.17; KataGo): self-play records every "
                    "row's KL(pi || the net's raw prior) and the training batches draw row i in proportion to --surprise-uniform + "
                    "(1 - --surprise-uniform) kl_i / mean kl (rows are repeated in the data, not reweighted in the loss); validation rows "
                    "are not resampled")
    ap.add_argument("--surprise-uniform", type=float, default=0.5, help="the share of the weight every row gets regardless of its "
                    "surprise (KataGo's 0.5)")
    ap.add_argument("--value-lambda", type=float, default=None, help="search-value targets (DESIGN.md 3.18): the value head trains on the "
                    "TD(lambda) return bootstrapped from the later roots' search values instead of the game's outcome; 1 = the outcome, "
                    "0 = the next recorded root's value.  Switches the recording of the root value on")
    ap.add_argument("--value-q-mix", type=float, default=None, help="search-value targets: the weight of the row's own root value in the "
                    "target, (1 - M) * return + M * q; 0.5 at --value-lambda 1 averages z and q.  Switches the recording on")
    ap.add_argument("--eval-symmetry", action="store_true", help="self-play evaluates every leaf under a hashed board symmetry (DESIGN.md "
                    "3.19; AlphaGo Zero, KataGo), seeded with --seed + the iteration, so a position's orientation changes from net to net; "
                    "the arena and gate players run plain, and the validation line also reports the symmetrised (mean over the eight) net")
    ap.add_argument("--fpu-reduction", type=float, default=None, help="first-play urgency reduction (DESIGN.md 3.20; KataGo uses 0.2): the "
                    "select rule scores a child that was never visited with its parent's value minus R sqrt(visited prior mass) instead of "
                    "with 0, in self-play, for both players of the gate and for the arena's search player; not given = off (0 is a "
                    "reduction).  Not with --gumbel")
    ap.add_argument("--fpu-root-reduction", type=float, default=0.1, help="the reduction at the root under --fpu-reduction (KataGo's 0.1)")
    ap.add_argument("--solver", action="store_true", help="proven wins, losses and draws (DESIGN.md 3.23) in self-play, for both players "
                    "of the gate and for the arena's search player.  Not with --gumbel, --forced-k or --fpu-reduction")
    ap.add_argument("--early-stop", action="store_true", help="exact early stop (DESIGN.md 3.25) for both players of the gate and for "
                    "the arena's search player: a search stops once the simulations left cannot change its move, and plays the "
                    "move the full search plays.  Never in self-play (a shortened search changes pi).  Not with --gumbel or --solver")
    ap.add_argument("--gate-games", type=int, default=0, help="games (even) of the match between the freshly trained net and the net "
                    "self-play uses, at --arena-sims and --opening-plies; 0 = no gate: every trained net goes to self-play")
    ap.add_argument("--gate-score", type=float, default=0.55, help="the candidate is promoted at a match score >= this (AlphaGo Zero's 55 %%)")
    ap.add_argument("--weight-decay", type=float, default=0.0, help="AdamW's decoupled weight decay on the weights (not the biases) of "
                    "the all-kernel step (GraphedTrainStep.weight_decay)")
    ap.add_argument("--clip-norm", type=float, default=0.0, help="clip the global gradient norm of every step at this value (0: off)")
    ap.add_argument("--ema-decay", type=float, default=None, help="keep an exponential moving average of the weights with this decay; the "
                    "net that is validated, gated and pushed to the engine is then the averaged one")
    ap.add_argument("--lr-decay", type=float, default=1.0, help="the learning rate is multiplied by this after every iteration "
                    "(GraphedTrainStep.set_lr: no recapture)")
    ap.add_argument("--ownership", action="store_true", help="ownership targets (DESIGN.md 3.22, 12.2; KataGo): self-play keeps every "
                    "game's final board, and an auxiliary head next to the net learns, per cell, who owns it at the end; the head "
                    "only shapes the trunk, the engine's net does not have it.  Needs the all-kernel training step")
    ap.add_argument("--own-weight", type=float, default=1.0, help="the weight of the ownership loss in the step's loss (untuned)")
    ap.add_argument("--resign-threshold", type=float, default=None, help="resignation in self-play (DESIGN.md 3.24; AlphaGo Zero): a side "
                    "whose root value stayed below T for --resign-consecutive full searches in a row resigns; not given = every game is "
                    "played to the end.  After an iteration with played-out games that would have resigned, T moves down by "
                    f"{RESIGN_STEP_DOWN} when their false-positive rate is above --resign-fp-target and up by {RESIGN_STEP_UP} when it "
                    f"is below half of it, inside [{RESIGN_T_MIN}, {RESIGN_T_MAX}] (the two steps are untuned).  Not with --ownership")
    ap.add_argument("--resign-consecutive", type=int, default=2, help="full searches in a row below the threshold before a side resigns")
    ap.add_argument("--resign-playout-frac", type=float, default=0.1, help="the share of the games that never resigns and records where "
                    "it would have (AlphaGo Zero's 10 %%): the false-positive rate is measured on them")
    ap.add_argument("--resign-fp-target", type=float, default=0.05, help="the false-positive rate the threshold is steered to stay "
                    "under (AlphaGo Zero's 5 %%)")
    ap.add_argument("--merge-positions", action="store_true", help="position averaging (DESIGN.md 3.26; AlphaZero.jl): once per iteration "
                    "the rows of the augmented training window that share a position become one row with the mean pi and the mean value "
                    "target (the step then trains on float value targets); the held-out rows stay as they are.  Not with --ownership")
    ap.add_argument("--merge-weight", choices=("constant", "log"), default="constant", help="under --merge-positions: how often a merged "
                    "row of n rows stands in the list the batches are drawn from: once, or 1 + floor(log2 n) times (not with --surprise)")
    ap.add_argument("--fp8", action="store_true", help="the fp8 net in the loop (DESIGN.md 12.3): self-play, the gate match and the "
                    "arena run on net_fp8, and the training step is quantisation-aware (GraphedTrainStep(fp8_qat=True): the fp8 net's "
                    "forward, straight-through gradients).  Needs --channels 128 and the all-kernel training step")
    ap.add_argument("--fp8-no-qat", action="store_true", help="under --fp8: keep the plain bf16 training step (the ablation: fp8 "
                    "self-play on post-training-quantised weights)")
    ap.add_argument("--reanalyse-frac", type=float, default=0.0, help="reanalysis (DESIGN.md 3.27; MuZero Reanalyse): every iteration, after "
                    "self-play and before training, this share of the training rows of every window slot older than the current one is "
                    "searched again with the net self-play just used and self-play's search options (no noise, no playout cap, no "
                    "resignation), and gets that search's pi (and kl under --surprise); the value targets stay, the held-out rows are "
                    "never touched; 0 = off")
    ap.add_argument("--train-symmetry", action="store_true", help="a board symmetry per row inside the training step (DESIGN.md 12.5; "
                    "AlphaGo Zero's per-position rotation / reflection): the window holds the training rows as played -- no eightfold "
                    "copy, no dedupe, no re-augmentation after reanalysis -- and every step draws one of the eight symmetries per batch "
                    "position from the generator that draws the rows; an epoch is 8 * rows / batch steps, so --epochs keeps its meaning.  "
                    "--merge-positions then merges exact repeats only (symmetric copies of a position no longer meet).  Needs the "
                    "all-kernel training step")
    ap.add_argument("--reanalyse-sims", type=int, default=None, help="simulations of a reanalysis search (default: --sims)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fp32-train", action="store_true", help="train without bf16 autocast (A/B of the loss curve)")
    ap.add_argument("--eager-train", action="store_true", help="launch every kernel of a training step by itself instead of replaying the captured HIP graph")
    ap.add_argument("--miopen-train", action="store_true", help="train the tower through stock autograd (MIOpen) instead of the HIP training kernels (csrc/bz_train.hip)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--save-net", default=None, help="write the state_dict of the net training ends with to this file (what the "
                    "bench tools' --net takes)")
    ap.add_argument("--checkpoint", default=None, metavar="PATH", help="write the run's whole state to this file (DESIGN.md 12.4; "
                    "betazero_amd.checkpoint: one file, replaced atomically) after every --checkpoint-every'th completed iteration and "
                    "after the last one")
    ap.add_argument("--checkpoint-every", type=int, default=1, help="iterations between two checkpoints")
    ap.add_argument("--no-checkpoint-window", action="store_true", help="leave the training window out of the checkpoint (a much "
                    "smaller file); a run resumed from it starts with an empty window and is NOT the uninterrupted run bit for bit")
    ap.add_argument("--resume", default=None, metavar="PATH", help="continue the run of this checkpoint up to --iters: with the "
                    "all-kernel training step the resumed run is the uninterrupted run bit for bit.  Every argument but --iters, "
                    "--out, --save-net and the checkpoint flags must be the checkpoint's")
    ap.add_argument("--init-net", default=None, metavar="FILE", help="start a new run from this saved state_dict (what --save-net "
                    "writes) instead of random weights")
    return ap


def window_rows(ex):
    """DeviceExamples -> {column: CPU tensor} (+ the board size), every column the rows carry: what a checkpoint keeps of a
    window slot"""
    from betazero_amd.examples import columns
    return {"size": int(ex.size), **{k: t.cpu() for k, t in columns(ex).items()}}


def to_host(x):
    """tensors anywhere inside dicts / lists / tuples -> CPU tensors, tuples -> lists: what a checkpoint holds"""
    if torch.is_tensor(x):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: to_host(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [to_host(v) for v in x]
    return x


def rows_to_device(rows, device="cuda:0"):
    from betazero_amd.examples import DeviceExamples
    return DeviceExamples(**{k: (v if k == "size" else v.to(device)) for k, v in rows.items()})


def main():
    ap = build_parser()
    args = ap.parse_args()
    ckpt = None
    if args.checkpoint_every < 1:
        ap.error("--checkpoint-every must be >= 1")
    if args.resume and args.init_net:
        ap.error("--init-net starts a new run; --resume continues one")
    if args.resume:  # read and checked on the host: a checkpoint that does not fit is refused before any device is touched
        from betazero_amd.checkpoint import load_checkpoint
        try:
            ckpt = load_checkpoint(args.resume)
        except (OSError, ValueError) as e:
            ap.error(f"--resume: {e}")
        saved = ckpt.get("args")
        if not isinstance(saved, dict) or "iter" not in ckpt:
            ap.error(f"--resume: {args.resume} is not a checkpoint of this tool")
        for k, v in vars(args).items():
            if k not in RESUME_FREE and (k not in saved or saved[k] != v):
                ap.error(f"--resume: --{k.replace('_', '-')} differs from the checkpoint's: it was written with "
                         f"{saved.get(k, 'no such argument')!r}, this run has {v!r}")
        if ckpt["iter"] > args.iters:
            ap.error(f"--resume: the checkpoint has completed iteration {ckpt['iter']}, --iters is {args.iters}")
    if not (0.0 <= args.reanalyse_frac <= 1.0):
        ap.error("--reanalyse-frac must be in [0, 1]")
    if args.reanalyse_sims is not None and not args.reanalyse_frac > 0:
        ap.error("--reanalyse-sims takes effect only with --reanalyse-frac")
    if args.reanalyse_sims is not None and args.reanalyse_sims < 1:
        ap.error("--reanalyse-sims must be >= 1")
    if args.gumbel_interior and not args.gumbel:
        ap.error("--gumbel-interior takes effect only with --gumbel")
    extended = bool(args.weight_decay or args.clip_norm or args.ema_decay is not None)
    if (extended or args.lr_decay != 1.0) and (args.miopen_train or args.eager_train or args.fp32_train or args.channels == 256):
        ap.error("--weight-decay / --clip-norm / --ema-decay / --lr-decay need the all-kernel training step")
    if args.ownership and (args.miopen_train or args.eager_train or args.fp32_train or args.channels == 256):
        ap.error("--ownership needs the all-kernel training step")
    if args.train_symmetry and (args.miopen_train or args.eager_train or args.fp32_train or args.channels == 256):
        ap.error("--train-symmetry needs the all-kernel training step")
    if args.resign_threshold is not None and args.ownership:
        ap.error("--resign-threshold does not combine with --ownership: a resigned game has no final board")
    if args.merge_positions and args.ownership:
        ap.error("--merge-positions does not combine with --ownership: the ownership targets are boards and have no mean")
    if args.merge_weight != "constant" and not args.merge_positions:
        ap.error("--merge-weight takes effect only with --merge-positions")
    if args.merge_positions and args.merge_weight == "log" and args.surprise:
        ap.error("--merge-weight log does not combine with --surprise: both repeat rows in the list the batches are drawn from")
    if not (0.0 <= args.resign_fp_target <= 1.0):
        ap.error("--resign-fp-target must be in [0, 1]")
    if not (0.0 <= args.own_weight < float("inf")):
        ap.error("--own-weight must be finite and >= 0")
    if args.fp8_no_qat and not args.fp8:
        ap.error("--fp8-no-qat takes effect only with --fp8")
    if args.fp8 and args.channels != 128:
        ap.error("--fp8 needs --channels 128: the fp8 tower is built for 128 channels")
    if args.fp8 and not args.fp8_no_qat and (args.miopen_train or args.eager_train or args.fp32_train):
        ap.error("--fp8 trains with the all-kernel step (quantisation-aware); --fp8-no-qat keeps any other step")
    net_eval = "net_fp8" if args.fp8 else "net_bf16"   # the evaluator of self-play, the gate and the arena
    fp8_qat = args.fp8 and not args.fp8_no_qat

    torch.manual_seed(args.seed)
    gen = torch.Generator(device="cuda:0").manual_seed(args.seed)
    use_vt = args.value_lambda is not None or args.value_q_mix is not None
    train_vt = use_vt or args.merge_positions   # merged rows carry float value targets
    v_lam, v_mix = 1.0 if args.value_lambda is None else args.value_lambda, 0.0 if args.value_q_mix is None else args.value_q_mix
    kernels = not (args.miopen_train or args.eager_train or args.fp32_train or args.channels == 256)
    module = PolicyValueNet(args.channels, args.blocks, 64, fused_tower=kernels)
    if args.init_net:
        module.load_state_dict(torch.load(args.init_net, map_location="cpu", weights_only=True))
    own_head = OwnershipHead(args.channels) if args.ownership else None
    opt = make_optimizer(module, lr=args.lr) if args.eager_train else None
    graphed = None if args.eager_train else GraphedTrainStep(module, lr=args.lr, batch=args.batch, autocast=not args.fp32_train, lr_warmup_steps=args.lr_warmup,
                                                                  value_targets=train_vt, weight_decay=args.weight_decay, clip_norm=args.clip_norm,
                                                                  ema_decay=args.ema_decay, ownership=own_head, own_weight=args.own_weight,
                                                                  fp8_qat=fp8_qat, symmetry=args.train_symmetry)
    bmax = max(args.games, args.arena_games, args.gate_games)
    if ckpt is not None:  # the trained state: the step's (parameters, optimiser, EMA, ownership head), or torch's where it trained
        with torch.no_grad():
            for k, p in module.state_dict().items():
                p.copy_(ckpt["module"][k])
            if own_head is not None:
                for k, p in own_head.state_dict().items():
                    p.copy_(ckpt["own_head"][k])
        if graphed is not None:
            graphed.load_state_dict(ckpt["step"])
        else:  # (torch's optimiser keeps its state where the parameters are when it is loaded)
            module.to("cuda:0")
            opt.load_state_dict(ckpt["optimizer"])
        gen.set_state(ckpt["generator"])
    # the net self-play uses, as the flat bf16-representable vector it was last given (a DeviceNet cannot be read back)
    dnet_flat = ckpt["dnet"].numpy() if ckpt is not None else module.round_to_bf16_().flat_params()
    dnet = DeviceNet(args.channels, args.blocks, 64, dnet_flat, bmax)
    # with the gate on, the freshly trained weights live in a net of their own until they have won their match
    cand = DeviceNet.from_module(module, bmax) if args.gate_games else dnet
    gumbel = GumbelConfig(interior="gumbel" if args.gumbel_interior else "puct") if args.gumbel else None
    cap = check_playout_cap(PlayoutCap(args.fast_sims, args.full_prob) if args.fast_sims else None, args.sims, gumbel=gumbel)
    forced = check_forced_playouts(ForcedPlayouts(args.forced_k, not args.no_prune) if args.forced_k else None, gumbel=gumbel)
    fpu = check_fpu(Fpu(args.fpu_reduction, args.fpu_root_reduction) if args.fpu_reduction is not None else None, gumbel=gumbel)
    solver = check_solver(args.solver, gumbel=gumbel, forced_playouts=forced, fpu=fpu)
    resign = check_resign(Resign(args.resign_threshold, args.resign_consecutive, args.resign_playout_frac)
                          if args.resign_threshold is not None else None, ownership=args.ownership)
    early_stop = check_early_stop(args.early_stop, gumbel=gumbel, solver=solver)  # the gate's and the arena's players only
    lines = list(ckpt["lines"]) if ckpt is not None else []
    if ckpt is not None and resign is not None:
        resign = check_resign(Resign(ckpt["resign_threshold"], resign.consecutive, resign.playout_frac))

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    def arena(evaluator, net, depth=None):
        t0 = time.time()
        try:
            res = play_arena("reversi", args.arena_games, args.arena_sims, opponent_depth=depth or args.depth, evaluator=evaluator,
                             net=net, seed=args.seed, opening_plies=args.opening_plies, gumbel=gumbel, fpu=fpu, solver=solver,
                             early_stop=early_stop)
        except RuntimeError:  # keep the weights that were in play for a post-mortem
            if args.out:
                np.save(args.out + ".failed_params.npy", module.flat_params())
            raise
        s = res.summary()
        s["score"] = round((s["wins"] + 0.5 * s["draws"]) / s["games"], 4)
        s["seconds"] = round(time.time() - t0, 1)
        return s

    if ckpt is None:  # (a resumed run has these two lines in the checkpoint's)
        emit({"what": "arena, MCTS with the uniform evaluator (no net)", "sims": args.arena_sims, "opponent_depth": args.depth,
              **arena("uniform", None)})
        emit({"what": "arena, untrained net", "iter": 0, "evaluator": net_eval, **arena(net_eval, dnet)})

    window, val_window = [], []
    # --train-symmetry: the rows as played ARE the window (the symmetries are drawn per step); otherwise the eightfold copy, deduped
    augment = (lambda rows: rows) if args.train_symmetry else (lambda rows: augment_examples(rows, dedupe=True))
    sym_fold = 8 if args.train_symmetry else 1   # steps per row of the window, so that an epoch is what it is without the flag
    # what a checkpoint keeps of the window: every slot's rows BEFORE augmentation (an eighth of the augmented rows), on the host
    keep_rows = bool(args.checkpoint) and not args.no_checkpoint_window
    raw_window = []
    # reanalysis: every slot's un-augmented training rows stay on the device, next to the slot they augment to
    reanalysing = args.reanalyse_frac > 0
    raw_dev = []
    rean = None
    if ckpt is not None and ckpt.get("window") is not None:   # augmentation and dedupe are deterministic: the same window again
        raw_window = list(ckpt["window"]) if keep_rows else []
        window = [augment(rows_to_device(w["train"])) for w in ckpt["window"]]
        if reanalysing:   # (under --train-symmetry the very tensors of the window: reanalysis rewrites them in place)
            raw_dev = list(window) if args.train_symmetry else [rows_to_device(w["train"]) for w in ckpt["window"]]
        val_window = [rows_to_device(w["val"]) for w in ckpt["window"]]

    def write_checkpoint(it):
        from betazero_amd.checkpoint import save_checkpoint
        save_checkpoint(args.checkpoint, to_host({
            "iter": it, "args": vars(args), "lines": lines, "module": dict(module.state_dict()),
            "own_head": dict(own_head.state_dict()) if own_head is not None else None,
            "step": graphed.state_dict() if graphed is not None else None,
            "optimizer": opt.state_dict() if opt is not None else None,
            "dnet": torch.from_numpy(np.ascontiguousarray(dnet_flat, dtype=np.float32)), "generator": gen.get_state(),
            "resign_threshold": resign.threshold if resign is not None else None,
            "window": raw_window if keep_rows else None}))

    for it in range((ckpt["iter"] if ckpt is not None else 0) + 1, args.iters + 1):
        t0 = time.time()
        sp = PipelinedSelfPlay("reversi", args.games, args.sims, net_eval, dnet, pipelines=args.pipelines, temp_moves=args.temp_moves,
                               openings=1, seed=args.seed * 1000 + it, gumbel=gumbel, playout_cap=cap, forced_playouts=forced,
                               surprise=args.surprise, search_value=use_vt, fpu=fpu, solver=solver, ownership=args.ownership, resign=resign,
                               eval_symmetry=EvalSymmetry(args.seed + it) if args.eval_symmetry else None, **({} if args.gumbel else dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)))
        plies = sp.run_iteration()
        ex = sp.device_examples()    # finished games' rows, packed on the device
        vt_info = {}
        if use_vt:  # while every game's rows stand together in ply order: before the split and the augmentation
            ex = value_targets(ex, v_lam, v_mix)
            vt_info = {"value_targets": {"lambda": v_lam, "q_mix": v_mix,
                                         "mean_abs_vt_minus_z": round(float((ex.vt - ex.z.to(torch.float32)).abs().mean()), 5)}}
        winners, _ = sp.winners()
        cnt = sp.counters()
        resign_info = {}
        if resign is not None:  # this iteration's figures, then the next iteration's threshold
            st = sp.resign_stats()
            nxt = next_resign_threshold(resign.threshold, st, args.resign_fp_target)
            resign_info = {"resign": {"threshold": round(resign.threshold, 4), "consecutive": resign.consecutive,
                                      "playout_frac": resign.playout_frac, **st, "next_threshold": round(nxt, 4)}}
            resign = check_resign(Resign(nxt, resign.consecutive, resign.playout_frac))
        torch.cuda.synchronize()
        t_play = time.time() - t0
        rean_info = {}
        if reanalysing:  # the older slots that stay in the window, with the net that just played (dnet) and self-play's search
            t_re = time.time()
            if rean is None:
                rean = Reanalyser("reversi", args.reanalyse_sims or args.sims, net_eval, dnet, batch=max(1, min(1024, args.games // args.pipelines)),
                                  pipelines=args.pipelines, gumbel=gumbel, fpu=fpu, forced_playouts=forced, solver=solver,
                                  eval_symmetry=EvalSymmetry(args.seed + it) if args.eval_symmetry else None, seed=args.seed)
            elif args.eval_symmetry:
                for e in rean.engines:
                    e.set_eval_symmetry(EvalSymmetry(args.seed + it))
            keep = min(len(window), args.window - 1)   # the slots this iteration's rows do not push out
            n_re, n_moved = 0, torch.zeros((), dtype=torch.int64, device=ex.own.device)
            for j in range(len(window) - keep, len(window)):
                raw = raw_dev[j]
                idx = reanalyse_rows(len(raw), args.reanalyse_frac, args.seed, (it, len(window) - j)).to(raw.own.device)
                if len(idx) == 0:
                    continue
                top = raw.pi[idx].argmax(1)
                rean.run(raw, idx, update_q=False)   # the slot's value targets were computed over whole games and stay
                n_moved += (raw.pi[idx].argmax(1) != top).sum()
                n_re += len(idx)
                window[j] = augment(raw)
                if keep_rows:
                    raw_window[j] = {"train": window_rows(raw), "val": raw_window[j]["val"]}
            torch.cuda.synchronize()
            rean_info = {"reanalysed_rows": n_re, "reanalyse_s": round(time.time() - t_re, 1),
                         "reanalyse_argmax_changed": round(int(n_moved) / n_re, 4) if n_re else 0.0}
        t1 = time.time()
        # hold-out split of this iteration's rows BEFORE augmentation (a row's symmetric copies must not sit on both sides)
        tr_idx, va_idx = holdout_split(len(ex), args.val_split, gen, ex.own.device)
        tr_rows, va_rows = select_rows(ex, tr_idx), select_rows(ex, va_idx)
        aug = augment(tr_rows)
        del sp
        window = (window + [aug])[-args.window:]
        if reanalysing:
            raw_dev = (raw_dev + [tr_rows])[-args.window:]
        val_window = (val_window + [va_rows])[-args.window:]
        if keep_rows:
            raw_window = (raw_window + [{"train": window_rows(tr_rows), "val": window_rows(va_rows)}])[-args.window:]
        data, val = concat_device_examples(window), concat_device_examples(val_window)
        val_before = validate(dnet, val, fp8=args.fp8)   # the net that just played, on rows it has not been trained on
        steps = max(1, int(args.epochs * sym_fold * len(data) / args.batch))
        losses = []
        surprise = {}
        res = None
        merge_info = {}
        if args.merge_positions:  # once per iteration, over the window; the held-out rows stay unmerged
            rows_before = len(data)
            data, counts = merge_positions(data, return_counts=True)
            steps = max(1, int(args.epochs * sym_fold * len(data) / args.batch))   # an epoch is a pass over the merged rows
            if args.merge_weight == "log":
                res = merged_repeats(counts, "log")
            merge_info = {"merge": {"rows_before": rows_before, "rows_after": len(data), "largest_group": int(counts.max()),
                                    "share_rows_in_groups": round(float(counts[counts > 1].sum()) / rows_before, 4),
                                    "weight": args.merge_weight}}
        if args.surprise:  # once per iteration, over the window: row i stands count_i times in res
            res, counts = surprise_resample(data, args.surprise_uniform, seed=args.seed * 1000 + it, return_counts=True)
            surprise = {"surprise": {"mean_kl": round(float(data.kl.mean()), 5), "resampled_over_rows": round(len(res) / len(data), 4),
                                     "max_count": int(counts.max()), "share_count_0": round(float((counts == 0).float().mean()), 4),
                                     "uniform": args.surprise_uniform}}
        for _ in range(steps):
            idx = torch.randint(0, len(data) if res is None else len(res), (args.batch,), device=data.own.device, generator=gen)
            if res is not None:
                idx = res[idx]
            if args.train_symmetry:   # the same generator as the rows: a resumed run draws what the uninterrupted one draws
                sym = torch.randint(0, 8, (args.batch,), dtype=torch.uint8, device=data.own.device, generator=gen)
                losses.append(graphed(data, idx, sym))
            elif graphed is not None:
                losses.append(graphed(data, idx))
            else:
                losses.append(torch.stack(train_step(module, opt, data, idx, autocast=not args.fp32_train, value_targets=train_vt)))
        # the weights' fingerprint: the sum of the trained parameters' bit patterns (as int32) in 64 bits, computed on the device
        # and brought over with the losses -- as two more floats' bits, so that it stays one transfer
        whash = torch.stack([p.detach().reshape(-1).view(torch.int32).sum(dtype=torch.int64) for p in module.parameters()]).sum()
        losses = torch.stack(losses)
        packed = torch.cat([losses.reshape(-1), whash.reshape(1).view(torch.float32)]).cpu().numpy()  # one transfer per iteration
        losses, whash = packed[:-2].reshape(tuple(losses.shape)), int(packed[-2:].view(np.int64)[0])
        if graphed is not None:
            graphed.check()                         # an out-of-range row index in any step of the iteration raises here
        optim = {}
        if extended:  # a skipped step (non-finite gradient norm) left the weights as they were: reported, not fatal
            optim = {"optim": {**{k: (round(v, 5) if isinstance(v, float) else v) for k, v in graphed.optim_stats().items()},
                               "lr": graphed.lr}}
        bad = ~np.isfinite(losses).all(1)
        if extended and 0 < int(bad.sum()) <= optim["optim"]["skipped"]:   # the steps the optimiser refused: out of the means
            losses = losses[~bad] if not bad.all() else losses
        if not np.isfinite(losses).all():
            raise RuntimeError(f"training diverged in iteration {it}: first non-finite loss at step "
                               f"{int(np.argmax(~np.isfinite(losses).all(1)))} of {steps}")
        trained = graphed.ema_module() if args.ema_decay is not None else module   # the net that is validated, gated and played
        cand_flat = refresh_device_net(cand, trained)
        if not args.gate_games:
            dnet_flat = cand_flat
        if args.lr_decay != 1.0:
            graphed.set_lr(graphed.lr * args.lr_decay)
        t_train = time.time() - t1
        val_after = validate(cand, val, fp8=args.fp8)    # the refreshed engine net (bf16 MFMA forward) on the same held-out rows
        val_mean = {"after_mean_of_8": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in validate(cand, val, symmetry="mean", fp8=args.fp8).items()
                                        if k != "rows"}} if args.eval_symmetry else {}
        gate = {}
        if args.gate_games:  # the candidate (A) against the net self-play uses (B)
            t2 = time.time()
            res = play_match("reversi", args.gate_games, MatchPlayer(sims=args.arena_sims, net=cand, evaluator=net_eval, gumbel=gumbel, fpu=fpu,
                                                                             solver=solver, early_stop=early_stop),
                             MatchPlayer(sims=args.arena_sims, net=dnet, evaluator=net_eval, gumbel=gumbel, fpu=fpu, solver=solver, early_stop=early_stop), opening_plies=args.opening_plies,
                             seed=args.seed * 1000 + it)
            g = res.summary()
            g.update(promoted=bool(g["score"] >= args.gate_score), threshold=args.gate_score, seconds=round(time.time() - t2, 1))
            if g["promoted"]:
                dnet_flat = refresh_device_net(dnet, trained)
            gate = {"gate": g}
        head, tail = np.mean(losses[: max(1, steps // 10)], axis=0), np.mean(losses[-max(1, steps // 10):], axis=0)
        emit({"what": "iteration", "iter": it, "games": args.games, "plies": plies, "examples": int(len(ex)),
              "augmented_rows": int(len(aug)), "train_rows": int(len(data)), "steps": steps,
              "loss_first_tenth": [round(float(x), 4) for x in head], "loss_last_tenth": [round(float(x), 4) for x in tail],
              "weights_hash": f"{whash & 0xFFFFFFFFFFFFFFFF:016x}",
              "validation": {"rows": val_after["rows"], "split": args.val_split,
                             "before": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in val_before.items() if k != "rows"},
                             "after": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in val_after.items() if k != "rows"},
                             **val_mean},
              "self_play_x_wins": int((winners > 0).sum()), "self_play_o_wins": int((winners < 0).sum()),
              "self_play_s": round(t_play, 1), "games_per_s": round(args.games / t_play, 1),
              "rows_per_game": round(len(ex) / args.games, 2), "train_s": round(t_train, 1),
              **({"forced_k": forced.k, "prune": forced.prune} if forced else {}), **surprise, **vt_info, **resign_info, **merge_info, **rean_info,
              **({"fpu": [fpu.reduction, fpu.root_reduction]} if fpu else {}), **({"solver": True} if solver else {}), **optim,
              **({"gumbel_interior": gumbel.interior} if gumbel else {}),
              # the ownership loss L_own over the last (and the first) tenth of the steps
              **({"own": round(float(tail[3]), 4), "own_first_tenth": round(float(head[3]), 4), "own_weight": args.own_weight}
                 if args.ownership else {}),
              **({"eval_symmetry_seed": args.seed + it} if args.eval_symmetry else {}),
              "mean_walk_nodes": round(cnt["n_path_nodes"] / max(1, cnt["n_sims"]), 2),
              "evaluations_shared": round(cnt["n_cache_hits"] / max(1, cnt["n_cache_hits"] + cnt["n_net_leaves"]), 3),
              **({"fp8": True, "fp8_qat": fp8_qat} if args.fp8 else {}), **({"train_symmetry": True} if args.train_symmetry else {}),
              "arena": arena(net_eval, cand), **gate})
        if args.checkpoint and (it % args.checkpoint_every == 0 or it == args.iters):
            write_checkpoint(it)
    for d in (int(x) for x in args.final_depths.split(",") if x):
        emit({"what": "final arena", "opponent_depth": d, "sims": args.arena_sims, "trained": arena(net_eval, dnet, d),
              "uniform_evaluator": arena("uniform", None, d)})
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"args": vars(args), "lines": lines}, f, indent=1)
    if args.save_net:
        torch.save(module.state_dict(), args.save_net)


if __name__ == "__main__":
    main()
