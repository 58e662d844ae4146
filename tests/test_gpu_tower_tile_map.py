"""The edge-aware cell tiling of the 128-channel throughput tower (csrc/bz_tile_map.h): k_edge_bf16 deals a
wave's 256 (position, cell) pairs to its MFMA tiles so that the column taps skip whole tiles of halo reads too.  What it
skips are exact zeros and every output keeps its accumulation order, so every row must be the very bits that
k_tower_bf16 on board-row tiles gives (DeviceNet.set_tile_map(0)): with the host count at every ragged last workgroup, with
the device count through the adaptive pair, for random weights and for nets whose tower reads one conv tap only (a wrong
skip set, immediate or rotation of one tap cannot hide behind the other eight), on full, random and empty boards -- and
through the engine.  Nothing here has a tolerance, no row is left out."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
MAX_N = 512
HOST_COUNTS = (257, 258, 259, 260)
DEV_COUNT = 300
SENTINEL = -12345.0
_STATE = {}


def _boards():
    """{kind: (own, opp)} of MAX_N rows each: full boards (every square taken), random ones, empty ones"""
    if "boards" not in _STATE:
        rng = np.random.default_rng(5)
        split = rng.integers(0, 2 ** 64, MAX_N, dtype=np.uint64)
        occ = rng.integers(0, 2 ** 64, MAX_N, dtype=np.uint64) | rng.integers(0, 2 ** 64, MAX_N, dtype=np.uint64)
        full = np.full(MAX_N, 2 ** 64 - 1, dtype=np.uint64)
        dev = lambda a: torch.from_numpy(a.view(np.int64).copy()).cuda()  # noqa: E731
        _STATE["boards"] = {"full": (dev(full & split), dev(full & ~split)), "random": (dev(occ & split), dev(occ & ~split)),
                            "empty": (dev(np.zeros(MAX_N, np.uint64)), dev(np.zeros(MAX_N, np.uint64)))}
    return _STATE["boards"]


def _net(blocks, tap):
    """a DeviceNet of 128 channels with random bf16 weights; tap = 0..8: the tower's conv weights are zero except at that
    tap (and three times as large, so that the activations keep their spread)"""
    from betazero_amd.net import DeviceNet, PolicyValueNet
    torch.manual_seed(100 * blocks + (tap if tap is not None else 9))
    m = PolicyValueNet(128, blocks, 64)
    if tap is not None:
        with torch.no_grad():
            for conv in list(m.c1) + list(m.c2):
                keep = conv.weight[:, :, tap // 3, tap % 3].clone() * 3.0
                conv.weight.zero_()
                conv.weight[:, :, tap // 3, tap % 3] = keep
    return DeviceNet.from_module(m.round_to_bf16_(), MAX_N)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("tap", [None] + list(range(9)), ids=["random"] + [f"tap{t}" for t in range(9)])
@pytest.mark.parametrize("blocks", (1, 2))
def test_edge_tiling_gives_the_bits_of_the_row_tiles(blocks, tap):
    net = _net(blocks, tap)
    count = torch.full((1,), DEV_COUNT, dtype=torch.int32, device="cuda")
    sent = np.float32(SENTINEL).view(np.uint32)
    for kind, (own, opp) in _boards().items():
        for n in HOST_COUNTS:  # the throughput shape, 65 workgroups, the last one with 1, 2, 3 and 4 rows
            out = []
            for edge in (1, 0):
                net.set_tile_map(edge)
                lg, v = net.forward(own[:n].contiguous(), opp[:n].contiguous())
                out.append((_bits(lg), _bits(v)))
            assert np.isfinite(out[0][0].view(np.float32)).all() and np.isfinite(out[0][1].view(np.float32)).all()
            assert np.array_equal(out[0][0], out[1][0]), (kind, n)
            assert np.array_equal(out[0][1], out[1][1]), (kind, n)
            if kind == "random":  # the forward is not degenerate: rows differ from one another
                assert len(np.unique(out[0][1])) > n // 2
        out = []
        for edge in (1, 0):  # the adaptive pair: the latency window exits, the high window runs the throughput shape
            net.set_tile_map(edge)
            net.shape_tally()
            lg = torch.full((MAX_N, 65), SENTINEL, dtype=torch.float32, device="cuda")
            v = torch.full((MAX_N,), SENTINEL, dtype=torch.float32, device="cuda")
            net.forward_counted(own, opp, count, lg, v)
            assert net.shape_tally() == {"latency": 0, "middle": 0, "throughput": 1}, edge
            out.append((_bits(lg), _bits(v)))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), kind
        assert (out[0][0][DEV_COUNT:] == sent).all() and (out[0][1][DEV_COUNT:] == sent).all()
        assert not (out[0][0][:DEV_COUNT] == sent).any() and not (out[0][1][:DEV_COUNT] == sent).any()
    net.set_tile_map(1)


def _selfplay(net, edge):
    from betazero_amd.engine import SelfPlayEngine
    net.set_tile_map(edge)
    net.shape_tally()
    eng = SelfPlayEngine("reversi", 320, 24, "net_bf16", net=net, temp_moves=8, openings=1, seed=3, stagger=58, rounds=2,
                         eval_cache=True)  # (staggered starts: some games end within the three moves and leave example rows)
    eng.reset_games()
    for _ in range(3):
        eng.search()
        eng.play(True)
    eng.status()
    out = {"positions": eng.positions(), "examples": eng.examples(), "counters": eng.counters(), "tally": net.shape_tally()}
    net.set_tile_map(1)
    return out


def test_selfplay_is_identical_under_either_tile_map():
    from betazero_amd.net import DeviceNet, PolicyValueNet
    torch.manual_seed(11)
    net = DeviceNet.from_module(PolicyValueNet(128, 1, 64).round_to_bf16_(), 2048)
    on, off = _selfplay(net, 1), _selfplay(net, 0)
    print("tally on", on["tally"], "off", off["tally"], "counters", on["counters"], "rows", len(on["examples"]))
    assert on["tally"]["throughput"] > 0 and on["tally"] == off["tally"]  # the throughput shape ran, the same launches
    assert on["counters"] == off["counters"] and on["counters"]["n_net_leaves"] > 0
    for a, b in zip(on["positions"], off["positions"]):
        assert np.array_equal(a, b)
    ea, eb = on["examples"], off["examples"]
    assert len(ea) == len(eb) and len(ea) > 0
    for f in ("own", "opp", "pi", "z", "mover", "act", "game", "ply"):
        assert np.array_equal(getattr(ea, f), getattr(eb, f)), f
