"""References for the batch-API kernels (csrc/bz_env.hip, csrc/bz_arena.hip, betazero_amd/augment.py) and what of them can
be held to something without a GPU.  tests/test_gpu_batch_kernels.py imports the generators and references below and runs the
kernels against them; every comparison, here and there, is exact.

 * step_pool(size, n): seeded random well-formed Reversi positions of every density inside the size x size region with action
   bytes of every kind (legal placements, legal and illegal passes, occupied cells, empty cells that flip nothing, cells
   outside the region, bytes above 64), and the five outputs of one env step from the oracle's rule functions.
 * _minimax_ref: the decision rule of the reference's OptimalPlayer.minimax (reversi_players.py:41-69) restated over the
   oracle's bitboard functions, held to fixture F9; minimax_cases() / wide_rows() are the positions of the GPU test.
 * _first_occurrences (plain torch) with dishonest keys: the key-collision passes that honest keys never reach."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from oracle import oracle as orc

G = os.path.join(os.path.dirname(__file__), "golden")

# what an action byte is, for the coverage counts (K_LEGAL: the step is carried out)
K_LEGAL, K_BYTE, K_OUTSIDE, K_OCCUPIED, K_NOFLIP, K_PASS = range(6)
KIND_NAMES = ("legal", "byte > 64", "outside the region", "occupied cell", "flips nothing", "illegal pass")
ST_NAMES = {_lib.ST_RUNNING: "RUNNING", _lib.ST_TERMINAL: "TERMINAL", _lib.ST_ILLEGAL: "ILLEGAL", _lib.ST_MUST_PASS: "MUST_PASS"}
STEP_N = 20000       # rows per size in the GPU test
STRIDE_POOL = 4099   # a prime: coprime to the 4 games per lane, to the 256 lanes of a block and to the grid stride


def region(size):
    return sum(((1 << size) - 1) << (8 * r) for r in range(size))


def _u64s(rng, n):
    return rng.integers(0, 2**63, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, n).astype(np.uint64)


def _lowest(legal):
    return np.array([(int(l) & -int(l)).bit_length() - 1 if l else 64 for l in legal], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def step_pool(size, n=STEP_N):
    """n positions and action bytes at `size` (seed 100 + size) with the expected outputs of the env step: a dict of
    own / opp / act (inputs), own_next / opp_next / legal_next (u64, the NEXT mover's view), status (u8), winner (i8: the
    result for the player who just moved, 0 unless TERMINAL) and kind (K_*).  An illegal action leaves the position as it
    was and reports the mover's own legal mask, ILLEGAL and winner 0."""
    rng = np.random.default_rng(100 + size)
    reg = np.uint64(region(size))
    a, b = _u64s(rng, n), _u64s(rng, n)
    keep = np.full(n, ~np.uint64(0))
    for _ in range(3):  # thin out a share of the boards: a few stones to half a board per colour
        m = _u64s(rng, n)
        keep = np.where(rng.random(n) < 0.4, keep & m, keep)
    own, opp = a & ~b & keep & reg, b & ~a & keep & reg
    u = rng.random(n)  # fill a share of 0.35 of the boards up: most of them half of the empty cells, a fifth of them all
    extra = np.where(u < 0.35, ~(own | opp) & reg & np.where(u < 0.07, ~np.uint64(0), _u64s(rng, n)), np.uint64(0))
    own, opp = own | (extra & a), opp | (extra & ~a)
    assert not (own & opp).any() and not ((own | opp) & ~reg).any()
    legal = np.array([orc.reversi_legal(int(o), int(p), size) for o, p in zip(own, opp)], dtype=np.uint64)
    act = np.where(rng.random(n) < 0.5, rng.integers(0, 256, n), rng.integers(0, 65, n)).astype(np.uint8)
    act = np.where((rng.random(n) < 0.6) & (legal != 0), _lowest(legal), act).astype(np.uint8)
    act = np.where((legal == 0) & (rng.random(n) < 0.7), 64, act).astype(np.uint8)
    on, pn, lg = (np.zeros(n, np.uint64) for _ in range(3))
    st, w, kind = np.zeros(n, np.uint8), np.zeros(n, np.int8), np.zeros(n, np.uint8)
    for i in range(n):
        o, p, ac, l = int(own[i]), int(opp[i]), int(act[i]), int(legal[i])
        if ac == 64:
            k = K_LEGAL if l == 0 else K_PASS
        elif ac > 64:
            k = K_BYTE
        elif not (1 << ac) & int(reg):
            k = K_OUTSIDE
        elif (1 << ac) & (o | p):
            k = K_OCCUPIED
        else:
            k = K_LEGAL if l >> ac & 1 else K_NOFLIP
        kind[i] = k
        if k != K_LEGAL:
            if ac < 64:  # the oracle's make_move refuses what its legal mask lacks
                assert orc.reversi_apply(o, p, size, ac >> 3, ac & 7) is None, (size, i)
            on[i], pn[i], lg[i], st[i] = o, p, l, _lib.ST_ILLEGAL
            continue
        no, np_ = (p, o) if ac == 64 else orc.reversi_apply(o, p, size, ac >> 3, ac & 7)[:2][::-1]
        nl = orc.reversi_legal(no, np_, size)
        on[i], pn[i], lg[i] = no, np_, nl
        if nl == 0 and orc.reversi_game_over(no, np_, size):
            st[i], w[i] = _lib.ST_TERMINAL, orc.reversi_score(np_, no)[0]  # np_ = the stones of the player who just moved
        else:
            st[i] = _lib.ST_MUST_PASS if nl == 0 else _lib.ST_RUNNING
    return dict(size=size, own=own, opp=opp, act=act, legal=legal, own_next=on, opp_next=pn, legal_next=lg, status=st,
                winner=w, kind=kind)


def step_counts(pool):
    st = {name: int((pool["status"] == code).sum()) for code, name in ST_NAMES.items()}
    kinds = {KIND_NAMES[k]: int((pool["kind"] == k).sum()) for k in range(1, 6)}
    return st, kinds


def check_step_coverage(pool):
    """the issue's conditions on a pool of STEP_N rows, shown by the reference alone"""
    size = pool["size"]
    st, kinds = step_counts(pool)
    print(f"step pool size {size}: n = {len(pool['own'])} status {st} illegal kinds {kinds}")
    if size <= 2:  # no move ever exists on a 1x1 or 2x2 board
        assert st["RUNNING"] == 0 and st["MUST_PASS"] == 0 and st["TERMINAL"] > 100 and st["ILLEGAL"] > 100, st
        assert not pool["legal"].any() and kinds["illegal pass"] == 0 and min(kinds["byte > 64"], kinds["outside the region"]) >= 20
        return
    assert min(st.values()) >= 100, st
    assert min(v for k, v in kinds.items() if size < 8 or k != "outside the region") >= 20, kinds


def ttt_step_pool():
    """every position of ttt_exhaustive.npz x (the 9 cells and one byte of 9..255): inputs and the expected outputs of
    k_ttt_step from the oracle's rules; an occupied cell or a byte above 8 changes nothing and is ILLEGAL"""
    d = np.load(os.path.join(G, "ttt_exhaustive.npz"))
    pos = np.concatenate([d["pos"], d["extra"]])
    rng = np.random.default_rng(9)
    rows, exp = [], []
    for x, o, cur, legal, over, w1 in pos.tolist():
        tm = 1 if cur == 1 else -1
        own, opp = (x, o) if tm == 1 else (o, x)
        for a in list(range(9)) + [int(rng.integers(9, 256))]:
            rows.append((own, opp, a, tm))
            if a > 8 or (own | opp) >> a & 1:
                exp.append((own, opp, ~(own | opp) & 0x1FF, _lib.ST_ILLEGAL, 0))
                continue
            me = orc.ttt_apply(own, opp, a // 3, a % 3)
            nx, no = (me, opp) if tm == 1 else (opp, me)
            fin, win = orc.ttt_game_over(nx, no)
            exp.append((opp, me, orc.ttt_legal(nx, no), _lib.ST_TERMINAL if fin else _lib.ST_RUNNING, win if fin else 0))
    return np.array(rows, dtype=np.int64), np.array(exp, dtype=np.int64)


# ---------------------------------------------------------------- minimax
def _minimax_ref(self, other, size, max_depth, count=None, _depth=0):
    """OptimalPlayer.minimax (reversi_players.py:41-69) over the oracle's bitboard rules -> (move, score): `self` are the
    stones of the player, who moves at even depth.  No pass rule inside the search: a side without a move in an unfinished
    game scores -1000 (the player) / +1000 (the opponent) with move -1 (None); moves in ascending-bit order, the first
    strictly better one wins; the stone difference for the player at the depth limit or at game over.  count[0] += nodes."""
    if count is not None:
        count[0] += 1
    if _depth >= max_depth or orc.reversi_game_over(self, other, size):
        n_self, n_other = orc.reversi_score(self, other)[1]
        return -1, n_self - n_other
    maxi = _depth % 2 == 0
    moves = orc.reversi_legal(self, other, size) if maxi else orc.reversi_legal(other, self, size)
    best, best_move = (-1000, -1) if maxi else (1000, -1)
    while moves:
        a = (moves & -moves).bit_length() - 1
        moves &= moves - 1
        if maxi:
            s, o, _ = orc.reversi_apply(self, other, size, a >> 3, a & 7)
        else:
            o, s, _ = orc.reversi_apply(other, self, size, a >> 3, a & 7)
        sc = _minimax_ref(s, o, size, max_depth, count, _depth + 1)[1]
        if (sc > best) if maxi else (sc < best):
            best, best_move = sc, a
    return best_move, best


def _scalar(self, other, size, depth):
    mv, sc = C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().bz_reversi_minimax(self, other, size, depth, C.byref(mv), C.byref(sc)))
    return mv.value, sc.value


def _walk(rng, size, stop, every=False):
    """a seeded random game from the start position with the pass rule of reversi_terminal.py:31-35 -> (x, o) when
    stop(plies, empties) says so or the game is over; every=True: the list of all positions on the way, the last included"""
    p = size // 2 - 1
    x = (1 << (8 * p + p)) | (1 << (8 * (p + 1) + p + 1))
    o = (1 << (8 * p + p + 1)) | (1 << (8 * (p + 1) + p))
    cur, plies, seen = 1, 0, []
    while True:
        seen.append((x, o))
        if stop(plies, size * size - bin(x | o).count("1")):
            break
        own, opp = (x, o) if cur == 1 else (o, x)
        lg = orc.reversi_legal(own, opp, size)
        if not lg:
            cur, own, opp = -cur, opp, own
            lg = orc.reversi_legal(own, opp, size)
            if not lg:
                break  # finished
        cells = [i for i in range(64) if lg >> i & 1]
        a = cells[int(rng.integers(len(cells)))]
        own, opp, _ = orc.reversi_apply(own, opp, size, a >> 3, a & 7)
        x, o = (own, opp) if cur == 1 else (opp, own)
        cur, plies = -cur, plies + 1
    return seen if every else (x, o)


DEEP_EMPTIES = {4: 12, 6: 8, 8: 8}   # few empties keep depths 5..8 affordable for the Python reference
NODE_CAP = 500_000


@functools.lru_cache(maxsize=None)
def minimax_cases():
    """-> (rows, nodes): rows (size, depth, self, other, move, score, deeper) with move / score from _minimax_ref; deeper =
    the search one ply shallower decides otherwise (such a row tells depth from depth - 1: a kernel that loses its deepest
    level fails on it).  (a) depths 5..8 at sizes 4 / 6 / 8 on late positions, 7 per size and depth: 5 with depth ..
    DEEP_EMPTIES empties, so that lines of the full depth exist, 2 with 0 .. DEEP_EMPTIES (games walked to their end are
    among them); (b) depths 0..4 anywhere in the game, 6 per size and depth.  Both colours are `self`."""
    rng = np.random.default_rng(31)
    count, rows = [0], []
    for size in (4, 6, 8):
        for depth in range(9):
            for k in range(7 if depth >= 5 else 6):
                if depth >= 5:
                    e = int(rng.integers(depth if k < 5 else 0, DEEP_EMPTIES[size] + 1))
                    x, o = _walk(rng, size, lambda plies, empties: empties <= e)
                else:
                    t = int(rng.integers(0, size * size - 3))
                    x, o = _walk(rng, size, lambda plies, empties: plies >= t)
                s, ot = (x, o) if rng.integers(2) else (o, x)
                mv, sc = _minimax_ref(s, ot, size, depth, count)
                deeper = depth >= 1 and _minimax_ref(s, ot, size, depth - 1, count) != (mv, sc)
                rows.append((size, depth, s, ot, mv, sc, deeper))
    return tuple(rows), count[0]


@functools.lru_cache(maxsize=None)
def wide_rows():
    """a few thousand rows (size, depth, self, other) from the same walks: every position of 50 games per size, both colours;
    depths 0..8 once at most DEEP_EMPTIES empties are left, 0..4 (mostly 0..3) before"""
    rng = np.random.default_rng(32)
    rows = []
    for size in (4, 6, 8):
        for _ in range(50):
            for x, o in _walk(rng, size, lambda plies, empties: False, every=True):
                empties = size * size - bin(x | o).count("1")
                if empties <= DEEP_EMPTIES[size]:
                    depth = int(rng.integers(0, 9))
                else:
                    depth = int(rng.integers(0, 5 if rng.random() < 0.15 else 4))
                rows.append((size, depth) + ((x, o) if rng.integers(2) else (o, x)))
    return tuple(rows)


def test_minimax_ref_matches_every_reversi_row_of_fixture_f9():
    """the restatement against the decisions of the reference's own class (fixture F9, generated by importing it)"""
    rows = np.load(os.path.join(G, "minimax_players.npz"))["reversi"]
    count = [0]
    for size, depth, sym1, x, o, move, score in rows.tolist():
        s, ot = (x, o) if sym1 == 2 else (o, x)
        assert _minimax_ref(s, ot, size, depth, count) == (-1 if move == 255 else move, score - 2000), (size, depth, hex(x), hex(o))
    print("F9 reversi rows", len(rows), "reference nodes", count[0])


def test_minimax_cases_cover_the_quirks_and_the_scalar_entry_point_agrees():
    """the positions of the GPU test, by the reference alone: forced-pass rows (None, +-1000), depths 7 and 8, finished
    positions, both within the node budget; and bz_reversi_minimax -- the host build of the kernel's code -- on all of them"""
    rows, nodes = minimax_cases()
    live = [r for r in rows if r[1] >= 1 and not orc.reversi_game_over(r[2], r[3], r[0])]
    n_none = sum(r[4] == -1 for r in live)
    n_inf = sum(abs(r[5]) == 1000 for r in rows)
    n_over = sum(orc.reversi_game_over(r[2], r[3], r[0]) for r in rows)
    n_nomove = sum(orc.reversi_legal(r[2], r[3], r[0]) == 0 for r in live)
    per_depth = {d: sum(r[1] == d for r in rows) for d in range(9)}
    deeper = {d: sum(r[6] for r in rows if r[1] == d) for d in range(1, 9)}
    print(f"minimax cases: {len(rows)} rows, reference nodes {nodes}, move None (unfinished, depth >= 1) {n_none}, "
          f"score +-1000 {n_inf}, finished {n_over}, self without a move {n_nomove}, rows per depth {per_depth}, "
          f"of them decided otherwise one ply shallower {deeper}")
    assert nodes <= NODE_CAP, nodes
    assert n_none >= 5 and n_inf >= 10 and per_depth[7] >= 20 and per_depth[8] >= 20 and n_over >= 5 and n_nomove >= 5
    assert min(deeper.values()) >= 5, deeper  # every depth is told from the one before by several rows
    for size, depth, s, ot, mv, sc, _ in rows:
        assert _scalar(s, ot, size, depth) == (mv, sc), (size, depth, hex(s), hex(ot))


def test_wide_rows_are_a_few_thousand_over_every_size_and_depth():
    rows = wide_rows()
    groups = {}
    for size, depth, s, ot in rows:
        groups[(size, depth)] = groups.get((size, depth), 0) + 1
    print("wide rows", len(rows), "smallest (size, depth) group", min(groups.values()))
    assert len(rows) >= 2000 and set(groups) == {(s, d) for s in (4, 6, 8) for d in range(9)}


# ---------------------------------------------------------------- env step reference vs the scalar entry points
@pytest.mark.parametrize("size", range(1, 9))
def test_step_reference_agrees_with_the_scalar_rule_entry_points(size):
    """2,000 rows of the step recipe per size through bz_reversi_legal / _apply / _game_over (the host build of bz_rules.h):
    the legal mask, every refusal (occupied, flips nothing, outside the region) and the position after every placement"""
    pool = step_pool(size, 2000)
    L = _lib.lib()
    lg, a2, b2, fl, over = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int32()
    for i in range(2000):
        o, p, ac = int(pool["own"][i]), int(pool["opp"][i]), int(pool["act"][i])
        _lib.check(L.bz_reversi_legal(o, p, size, C.byref(lg)))
        assert lg.value == int(pool["legal"][i]), i
        if ac >= 64:
            continue
        rc = L.bz_reversi_apply(o, p, size, ac >> 3, ac & 7, C.byref(a2), C.byref(b2), C.byref(fl))
        if pool["kind"][i] != K_LEGAL:
            assert rc == _lib.BZ_EILLEGAL_MOVE, i
            continue
        assert rc == 0 and (b2.value, a2.value) == (int(pool["own_next"][i]), int(pool["opp_next"][i])), i
        _lib.check(L.bz_reversi_game_over(a2.value, b2.value, size, C.byref(over)))
        assert bool(over.value) == (pool["status"][i] == _lib.ST_TERMINAL), i


# ---------------------------------------------------------------- dedupe
def _dict_first(own, opp, pi):
    first = {}
    for i in range(len(own)):
        first.setdefault((int(own[i]), int(opp[i]), pi[i].tobytes()), i)
    return list(first.values())  # insertion order = ascending


def test_first_occurrences_is_exact_whatever_the_keys_do():
    """_first_occurrences on rows with exact copies, rows one ULP apart and +0 / -0 (distinct bit patterns), under keys that
    collide: all equal, i % 3, honest on half of the rows and one shared key on the rest.  Honest keys finish in one pass;
    these take the second and later passes.  The result is the dict's first-occurrence list whatever the keys are."""
    from betazero_amd.augment import _first_occurrences
    rng = np.random.default_rng(6)
    n, na = 301, 5
    own = rng.integers(-2**63, 2**63, n, dtype=np.int64)
    opp = rng.integers(-2**63, 2**63, n, dtype=np.int64)
    pi = rng.random((n, na)).astype(np.float32)
    for i in range(40, n):
        r = rng.random()
        j = int(rng.integers(0, i))
        if r < 0.35:      # an exact copy of an earlier row
            own[i], opp[i], pi[i] = own[j], opp[j], pi[j]
        elif r < 0.45:    # the boards of an earlier row, pi one ULP away
            own[i], opp[i], pi[i] = own[j], opp[j], pi[j]
            c = int(rng.integers(na))
            pi[i, c] = np.nextafter(pi[i, c], np.float32(2))
        elif r < 0.5:     # ... pi the same numbers, one zero of the other sign
            own[i], opp[i], pi[i] = own[j], opp[j], pi[j]
            pi[j, 1], pi[i, 1] = 0.0, -0.0
        elif r < 0.55:    # one board of an earlier row only
            own[i] = own[j]
    exp = _dict_first(own, opp, pi)
    assert 150 < len(exp) < n - 50
    honest = {}
    hk = np.array([honest.setdefault((int(a), int(b), p.tobytes()), len(honest)) for a, b, p in zip(own, opp, pi)], dtype=np.int64)
    keys = {"honest": hk, "all equal": np.zeros(n, np.int64), "i % 3": np.arange(n, dtype=np.int64) % 3,
            "half honest, half shared": np.where(np.arange(n) % 2 == 0, hk, -7),
            "two contents per key": hk // 2}
    t = torch.as_tensor
    for name, k in keys.items():
        got = _first_occurrences(t(k), t(own), t(opp), t(pi))
        assert got.dtype == torch.int64 and got.tolist() == exp, name
    assert _first_occurrences(t(hk[:0]), t(own[:0]), t(opp[:0]), t(pi[:0])).numel() == 0


def test_batch_entry_points_take_zero_rows_before_they_look_at_the_pointers():
    """an empty torch tensor hands a null data_ptr(): n == 0 is a no-op whatever the pointers are (az_loop can arrive with no
    finished game); n > 0 with a null pointer, a negative n and a bad size stay errors"""
    L = _lib.lib()
    assert L.bz_augment_d4_batch(None, None, None, 0, 8, 65, None, None, None, None, None) == _lib.BZ_OK
    assert L.bz_augment_d4_batch(None, None, None, 0, 3, 9, None, None, None, None, None) == _lib.BZ_OK
    assert L.bz_augment_d4_batch(None, None, None, 5, 8, 65, None, None, None, None, None) == _lib.BZ_EINVAL
    assert L.bz_augment_d4_batch(None, None, None, -1, 8, 65, None, None, None, None, None) == _lib.BZ_EINVAL
    assert L.bz_augment_d4_batch(None, None, None, 0, 5, 65, None, None, None, None, None) == _lib.BZ_EINVAL
    assert L.bz_augment_d4_batch(None, None, None, 0, 8, 63, None, None, None, None, None) == _lib.BZ_EINVAL
