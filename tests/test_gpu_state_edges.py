"""State rounds 16..31 and the exact ties of the median rule on every round
kernel, against the CPU oracle.

The packed state keeps B.round / C.rounds_in_state_b in a 5-bit field (planes
3..7, gs_common.h); max_rounds may be 32, so the field may reach 31, and the
kernels compare round + 1 >= max_rounds and round + 1 + rib >= max_rounds with
bit-sliced carry chains over those planes.  No other GPU test holds a B round
above 9 or a rib above 10: plane 7, the carry into it and out of it, and the
exits by the round limit at limits above 10 run only here.  The scenarios
(tests/state_edges.py) reach them through the public API alone:

* staggered injections under heavy drops: cells that hear little live through
  all max_rounds rounds -- the plain round kernels, faults on;
* peers outside the network with every internal batch dropped, so that every
  cell follows a script -- the kernels that apply external RPCs: a vote grid
  over every (|P|, ge) with |P| = 1..40 (across the 5-bit / 7-bit counter
  boundary, at both our_counter values, the ties 2 ge = |P| and one vote to
  either side included), and lifetimes that enter C at every rib 1..31.

Every round of every case: state, records, |P|, Statistics and known sets are
the oracle's; for the external RPCs the responses too.  What each scenario
covers, and the oracle itself at these rounds, are pinned on the CPU by
tests/test_state_edges_oracle.py.

All 32 cases passed on an MI355X the first time they ran: no kernel was wrong
at these rounds or ties.
"""
import pytest

import state_edges as se
from test_gpu_wire import _compare, _decode_batch, _key_sorted, _sharded, _sliced

pytestmark = pytest.mark.gpu

_ENV = ("SAFE_GOSSIP_AMD_DLV_PACK", "SAFE_GOSSIP_AMD_NO_DLV", "SAFE_GOSSIP_AMD_FILTER", "SAFE_GOSSIP_AMD_W32")


def _setenv(monkeypatch, env):
    for k, v in env.items():
        assert "SAFE_GOSSIP_AMD_" + k in _ENV
        monkeypatch.setenv("SAFE_GOSSIP_AMD_" + k, v)


_MAKES = {"single": None, "sliced2": _sliced(2), "sharded2x1": _sharded(2, 1), "sharded2x2": _sharded(2, 2)}


def _ids(cases):
    return ["-".join([str(c[0]), c[1]] + [k + v for k, v in c[2].items()] + [c[3]] * (c[3] != "single")) for c in cases]


def _make(engine, make, n, R, params, faults, schedule):
    make = _MAKES[make]
    kw = dict(churn=faults[0], drop_push=faults[1], drop_pull=faults[2])
    if schedule != "2P":
        kw["schedule"] = schedule
    return (make or engine.Network)(n, R, seed=se.SEED, params=params, **kw)


# ---------------------------------------------------------------- long-lived cells, no external RPCs

_STAGGERED = [
    ("500x16", "2P", {}, "single"),                                  # delivery records, two nodes per lane word
    ("500x16", "2P", {"DLV_PACK": "u64"}, "single"),
    ("500x16", "2P", {"DLV_PACK": "0"}, "single"),
    ("500x16", "2P", {"NO_DLV": "1"}, "single"),                     # small gather path
    ("500x16", "2P", {"NO_DLV": "1", "FILTER": "0"}, "single"),
    ("500x16", "SEQ", {}, "single"),
    ("999x7-churn", "2P", {}, "single"),                             # four nodes per lane word, churn freezes
    ("1030x1", "2P", {}, "single"),                                  # 16 lanes per word, ragged last word
    ("101x32", "2P", {}, "single"),                                  # the default 32-bit lane kernel
    ("300x64", "2P", {}, "single"),
    ("300x64", "SEQ", {}, "single"),
    ("300x64", "2P", {}, "sliced2"),
    ("300x64", "2P", {}, "sharded2x1"),                             # class rows
    ("130x256", "2P", {"W32": "1"}, "single"),
    ("130x256", "2P", {"W32": "0", "FILTER": "1"}, "single"),
    ("130x256", "2P", {"W32": "0", "FILTER": "0"}, "single"),
    ("500x16-max17", "2P", {}, "single"),                            # the limit on either side of plane 7
    ("500x16-max16", "2P", {}, "single"),
    ("500x16-cmax2", "2P", {}, "single"),
    ("500x16", "2P", {}, "sliced2"),
    ("5000x16", "2P", {}, "sharded2x2"),                            # code rows
]


@pytest.mark.parametrize("name,schedule,env,make", _STAGGERED, ids=_ids(_STAGGERED))
def test_staggered(engine, monkeypatch, name, schedule, env, make):
    _setenv(monkeypatch, env)
    n, R, params, faults = se.STAGGERED[name]
    net = _make(engine, make, n, R, params, faults, schedule)
    try:
        rounds = se.run_staggered(n, R, params, faults, schedule, net=net, compare=_compare)
    finally:
        net.close()
    assert rounds >= 7


# ---------------------------------------------------------------- scripted cells through external RPCs

def _hand_off(engine):
    def go(net, rpcs, exp):
        keys = {}
        wire = []
        for y, peer, push, rumor, ctr in rpcs:
            if rumor not in keys:
                keys[rumor] = b"" if rumor < 0 else net.rumor_key(rumor)
            wire.append((y, peer, engine.rpc_encode(not push, keys[rumor], ctr)))
        got = net.handle_received_batch(wire)
        assert len(got) == len(wire)
        for i, (g, e_) in enumerate(zip(got, exp)):
            if g or e_:  # (only a peer's first Push is answered)
                assert _decode_batch(engine, net, g, pull=True) == _key_sorted(net, e_), f"rpc {i} {rpcs[i]}"
    return go


_VOTES = [
    (64, "2P", {}, "single"),                    # gather path, 64-bit lanes: the full grid
    (64, "SEQ", {}, "single"),
    (32, "2P", {}, "single"),                    # the default 32-bit lane kernel
    (16, "2P", {}, "single"),                    # delivery records
    (16, "2P", {"DLV_PACK": "u64"}, "single"),
    (16, "2P", {"DLV_PACK": "0"}, "single"),
    (16, "2P", {"NO_DLV": "1"}, "single"),
    (64, "2P", {}, "sliced2"),
]


@pytest.mark.parametrize("R,schedule,env,make", _VOTES, ids=_ids(_VOTES))
def test_vote_grid(engine, monkeypatch, R, schedule, env, make):
    _setenv(monkeypatch, env)
    net = _make(engine, make, se.VOTE_N, R, se.VOTE_PARAMS, se.F_ALL, schedule)
    try:
        se.run_votes(R, schedule=schedule, net=net, compare=_compare, hand_off=_hand_off(engine))
    finally:
        net.close()


@pytest.mark.parametrize("R,schedule", [(64, "2P"), (64, "SEQ"), (16, "2P")])
def test_lifetimes(engine, R, schedule):
    net = _make(engine, "single", se.LIFE_N, R, se.LIFE_PARAMS, se.F_ALL, schedule)
    try:
        se.run_lifetimes(R, schedule=schedule, net=net, compare=_compare, hand_off=_hand_off(engine))
    finally:
        net.close()
