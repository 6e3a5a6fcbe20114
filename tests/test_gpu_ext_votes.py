"""Median votes of a hub node that many peers outside the simulated network
push to in one round (gs_handle_received[_batch]), against the CPU oracle.

Internal in-degrees stay below 31, so the round kernels' bit-sliced vote
counters are 5 bits wide; external RPCs have no such cap.  Here E = 31..100
distinct external peers hand one hub their copies, one vote pattern per rumor
column, so the recorded counts and |peers_in_this_round| cross 31 and 61 --
on every round-kernel path that applies external RPCs.  All integer work:
responses, state, records (c1 / c2 / anyC), |P|, Statistics and known sets
equal the oracle's (tests/test_oracle_many_peers.py pins the oracle itself at
these counts), straight after each hand-off and after every later round.
The engine bounds the recorded copies per (node, rumor) and round
(kExtCopiesMax = 96, GS_ERR_DEVICE_LIMIT); the last tests pin that bound.

With 5-bit counters in the kernels that apply external RPCs and no bound (the
state before this file was added), 34 of the 36 cases failed on an MI355X:
all but test_hub_gather[31] and test_hub_dlv[31], the last count 5 bits hold.
"""
import numpy as np
import pytest

from oracle_lib import SCHED_2P, SCHED_SEQ, OracleNet, fault_threshold
from test_gpu_parity import SEED
from test_gpu_wire import _compare, _decode_batch, _key_sorted, _sharded, _sliced

pytestmark = pytest.mark.gpu

PARAMS = (3, 3, 14)   # counters 1 and 2 are B votes, >= 3 acts as C
M_LIST = (15, 16, 17, 30, 31, 32, 33, 47, 48, 63, 64, 65, 95, 96)
COPIES_MAX = 96       # gs_common.h kExtCopiesMax
E_ALL = (31, 32, 33, 61, 62, 64, 100)
N_PULL = 10           # peers whose first RPC to the hub is a Pull copy


def _patterns(E, stage):
    """One vote pattern per rumor column: a list of per-column functions
    peer index -> [(counter, pull)] (the copies that peer sends, in order)."""
    ms = sorted({min(m, E) for m in M_LIST})
    cap = min(E, COPIES_MAX)  # the engine's bound on recorded copies per entry
    pats = []
    if stage == 1:  # the hub's entries are B with our_counter 1
        for m in ms:   # m of E peers vote ">= own"; the others 0-fill
            pats.append(lambda i, m=m: [(1, False)] if i < m else [])
        v = min(40, E - 1)  # one C copy on top of v ">=" votes: to C
        pats.append(lambda i, v=v: [(1, False)] if i < v else ([(255, False)] if i == v else []))
        k = min(33, E)      # the same peer twice: only its last copy is recorded
        pats.append(lambda i, k=k: [(0, False), (1, False)] if i == 0 else
                    ([(1, False), (0, False)] if i == 1 else ([(1, False)] if i < k else [])))
        # half the copies with counter 0 on the existing entry: recorded, vote "less"
        pats.append(lambda i: [(1 - (i & 1), False)] if i < cap else [])
        # copies arriving as Pull RPCs, the first RPC of their peers
        pats.append(lambda i: [(1, True)] if i >= E - N_PULL else [])
    else:  # some entries now have our_counter 2: counter 1 votes "less" there
        for q, m in enumerate(ms):
            a = ms[(q + 3) % len(ms)]     # copies with counter 2
            b = min(cap - a, 20 + q)      # copies with counter 1
            pats.append(lambda i, a=a, b=b: [(2, False)] if i < a else ([(1, False)] if i < a + b else []))
        pats.append(lambda i: [(2 - (i & 1), False)] if i < cap else [])
        pats.append(lambda i: [(2, True)] if i >= E - N_PULL else [])
        pats.append(lambda i: [(2, False), (1, False)] if i < 3 else ([(2, False)] if i < cap else []))
        pats.append(lambda i: [(255, False)] if i == E // 2 else ([(1, False)] if i < cap else []))
    return pats


def _slots(hubs, R, npat):
    """(hub, column) of every patterned entry, in pattern order (cyclic).  One
    wide hub: the columns spread over all its words, the last one included."""
    if len(hubs) == 1 and R >= npat:
        return [(hubs[0], k * (R - 1) // (npat - 1)) for k in range(npat)]
    return [(h, c) for h in hubs for c in range(R)]


def _rpcs(n, R, E, hubs, stage, order):
    """The stage's RPCs (hub, peer, push, rumor or -1, counter), peer by peer."""
    pats = _patterns(E, stage)
    slots = _slots(hubs, R, len(pats))
    out = []
    for i in order:
        for h in hubs:
            mine = []
            for k, (sh, c) in enumerate(slots):
                if sh == h:
                    mine += [(c, ctr, pull) for ctr, pull in pats[k % len(pats)](i)]
            mine.sort(key=lambda t: not t[2])  # (stable) a Pull copy goes first: it is the peer's first RPC
            if not mine:  # no copy for this hub: an empty Push (a peer of this round, 0-filled)
                out.append((h, n + 1 + i, True, -1, 0))
            out += [(h, n + 1 + i, not pull, c, ctr) for c, ctr, pull in mine]
    return out, slots


def _n_hubs(R, want=1):
    return max(want, -(-len(_patterns(100, 1)) // R))


def _hub_case(engine, n, R, E, make=None, schedule="2P", faults=None, batch=True, hubs=None):
    fk = dict(churn=faults[0], drop_push=faults[1], drop_pull=faults[2]) if faults else {}
    if schedule != "2P":
        fk["schedule"] = schedule
    osched = SCHED_SEQ if schedule == "SEQ" else SCHED_2P
    net = (make or engine.Network)(n, R, seed=SEED, params=PARAMS, **fk)
    orc = OracleNet(n, R, seed=SEED, params=PARAMS, faults=[fault_threshold(p) for p in faults] if faults else None)
    rng = np.random.default_rng(13 * n + R + E)
    nooff = np.zeros(n, dtype=bool)
    try:
        if faults:  # one hub online through the patterned rounds, one offline at the first hand-off
            offs = [orc.offline(r) for r in (1, 2, 3)]
            hubs = [int(np.flatnonzero(~(offs[0] | offs[1] | offs[2]))[0]), int(np.flatnonzero(offs[0])[0])]
        elif hubs is None:  # neighbours: the nodes of one lane word on the delivery-record path
            h0 = (n // 3) & ~3
            hubs = [h0 + q for q in range(_n_hubs(R))]
        for h in hubs:
            for r in range(R):
                net.send_new(h, r)
                orc.send_new(h, r)
        main = hubs[0]
        slots = None
        for rnd in range(1, 7):
            net.next_round()
            orc.next_round(osched)
            off = orc.offline(rnd) if faults else nooff
            if rnd == 2:
                # coverage, from the oracle alone: the median rule went both ways at the hub
                st = orc.dump_state()
                oc = {int(st[h, c]) >> 7 for h, c in slots if int(st[h, c]) >> 14 == 1}
                assert {(1 << 7) | 1, (1 << 7) | 2} <= oc, oc
            if rnd in (1, 2):
                if rnd == 1:
                    for h in hubs:
                        if not off[h]:
                            assert all(int(c) == (1 << 14) | (1 << 7) | 1 for c in orc.dump_state()[h])
                rpcs, slots = _rpcs(n, R, E, hubs, rnd, rng.permutation(E))
                wire, exp = [], []
                for y, peer, push, rumor, ctr in rpcs:
                    msg = b"" if rumor < 0 else net.rumor_key(rumor)
                    wire.append((y, peer, engine.rpc_encode(not push, msg, ctr)))
                    # a node offline this round drops every RPC to it
                    exp.append([] if off[y] else orc.receive(y, peer, push, rumor, ctr))
                got = net.handle_received_batch(wire) if batch else [net.handle_received(*w) for w in wire]
                assert len(got) == len(wire)
                for i, (g, e_) in enumerate(zip(got, exp)):
                    if g or e_:  # (only a peer's first Push is answered)
                        assert _decode_batch(engine, net, g, pull=True) == _key_sorted(net, e_), f"round {rnd} rpc {i}"
                # coverage: the counts go where the test means them to go
                orec, ops = orc.dump_records()
                top = max(max(int(orec[h, c]) & 0x7F, (int(orec[h, c]) >> 7) & 0x7F) for h, c in slots)
                assert min(E, COPIES_MAX) <= top < 128 and int(ops[main]) >= E
                if faults:  # the second hub is offline at the first hand-off: it drops everything
                    assert not off[main] and (rnd == 2 or off[hubs[1]])
            _compare(net, orc, off)
    finally:
        net.close()
        orc.close()


# ---------------------------------------------------------------- gather path, 64-bit lanes

@pytest.mark.parametrize("E", E_ALL)
def test_hub_gather(engine, E):
    _hub_case(engine, 250, 64, E)


def test_hub_gather_wide(engine):
    # patterned columns in all four words of the hub, the padded tail word included
    _hub_case(engine, 120, 200, 64)


def test_hub_gather_unfiltered_small(engine, monkeypatch):
    monkeypatch.setenv("SAFE_GOSSIP_AMD_FILTER", "0")
    monkeypatch.setenv("SAFE_GOSSIP_AMD_NO_DLV", "1")
    _hub_case(engine, 300, 16, 64)


# ---------------------------------------------------------------- 32-bit lane kernel

def test_hub_w32_default(engine):
    _hub_case(engine, 101, 32, 64)


def test_hub_w32_one_by_one(engine):
    # the same RPCs through gs_handle_received, one call each
    _hub_case(engine, 101, 32, 33, batch=False)


def test_hub_w32_forced(engine, monkeypatch):
    monkeypatch.setenv("SAFE_GOSSIP_AMD_W32", "1")
    _hub_case(engine, 130, 256, 64)


# ---------------------------------------------------------------- delivery records

@pytest.mark.parametrize("E", E_ALL)
def test_hub_dlv(engine, E):
    # two nodes per lane: the hub and its lane neighbour, both segments of
    # one lane word crossing 31 with different counts
    _hub_case(engine, 300, 16, E, hubs=[100, 101])


@pytest.mark.parametrize("n,R", [(999, 7), (1030, 1)])
def test_hub_dlv_four_per_lane(engine, n, R):
    _hub_case(engine, n, R, 64)


@pytest.mark.parametrize("pack", ["u64", "0"])
def test_hub_dlv_pack(engine, monkeypatch, pack):
    monkeypatch.setenv("SAFE_GOSSIP_AMD_DLV_PACK", pack)
    _hub_case(engine, 300, 16, 64, hubs=[100, 101])


# ---------------------------------------------------------------- SEQ, faults

@pytest.mark.parametrize("n,R", [(300, 16), (250, 64)])
def test_hub_seq(engine, n, R):
    _hub_case(engine, n, R, 64, schedule="SEQ")


def test_hub_faults(engine):
    _hub_case(engine, 120, 200, 64, faults=(0.05, 0.05, 0.05))


# ---------------------------------------------------------------- multi-engine, local transport

@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("n,R", [(250, 64), (300, 16)])
def test_hub_sliced(engine, world, n, R):
    _hub_case(engine, n, R, 64, make=_sliced(world))


def test_hub_sharded_class_rows(engine):
    _hub_case(engine, 250, 64, 64, make=_sharded(2, 1))


def test_hub_sharded_code_rows(engine):
    _hub_case(engine, 5000, 16, 64, make=_sharded(2, 2))


# ---------------------------------------------------------------- the bound on recorded copies

@pytest.mark.parametrize("make,n,R", [(None, 250, 64), (None, 300, 16), (_sliced(2), 300, 16),
                                      (_sharded(2, 1), 250, 64)],
                         ids=["gather", "dlv", "sliced", "sharded"])
def test_copies_bound(engine, make, n, R):
    """The 96th recorded copy of a (node, rumor) in a round is applied and
    exact; the 97th is refused with GS_ERR_DEVICE_LIMIT and nothing of its
    batch is applied; the round after is the oracle's, which never saw it."""
    net = (make or engine.Network)(n, R, seed=SEED, params=PARAMS)
    orc = OracleNet(n, R, seed=SEED, params=PARAMS)
    h, other, col = 40, 41, R - 1
    try:
        for x in (h, other):
            net.send_new(x, col)
            orc.send_new(x, col)
        net.next_round()
        orc.next_round(SCHED_2P)
        copy = engine.rpc_encode(False, net.rumor_key(col), 1)
        got = net.handle_received_batch([(h, n + 1 + i, copy) for i in range(COPIES_MAX)])
        for i, g in enumerate(got):
            assert _decode_batch(engine, net, g, pull=True) == _key_sorted(net, orc.receive(h, n + 1 + i, True, col, 1))
        orec, _ = orc.dump_records()
        assert int(orec[h, col]) & 0x7F == COPIES_MAX
        _compare(net, orc)
        st0 = net.statistics_all().copy()
        with pytest.raises(engine.DeviceError, match="status -5"):  # all or nothing
            net.handle_received_batch([(other, n + 500, copy), (h, n + 500, copy)])
        with pytest.raises(engine.DeviceError, match="status -5"):
            net.handle_received(h, n + 500, copy)
        np.testing.assert_array_equal(net.statistics_all(), st0)
        _compare(net, orc)
        # a peer that already has a recorded copy may replace it; another node is answered
        assert net.handle_received(h, n + 1, engine.rpc_encode(False, net.rumor_key(col), 0)) == []
        orc.receive(h, n + 1, True, col, 0)
        g = net.handle_received(other, n + 500, copy)
        assert _decode_batch(engine, net, g, pull=True) == _key_sorted(net, orc.receive(other, n + 500, True, col, 1))
        _compare(net, orc)
        for _ in range(2):
            net.next_round()
            orc.next_round(SCHED_2P)
            _compare(net, orc)
        # a new round: the count starts again
        net.handle_received(h, n + 500, copy)
        orc.receive(h, n + 500, True, col, 1)
        _compare(net, orc)
    finally:
        net.close()
        orc.close()
