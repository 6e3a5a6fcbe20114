"""The worklist of non-trivial waves (round_light + round_kernel<..., WL>;
DESIGN.md section 4) against the CPU oracle and against the full-grid path.

A deliver+transition launch of the 2P gather path (64 <= R_pad <= 512) may
run a light pass over all nodes -- a wave whose nodes are all-A, receive
nothing and get no injection only needs two Statistics increments per node --
and the round kernel over the remaining waves only.  Both ways must compute
the same, bit for bit: SAFE_GOSSIP_AMD_WORKLIST=1 forces the worklist wherever
it applies, =0 the full grid, unset lets the engine go over to the full grid
once many waves are listed.
"""
import numpy as np
import pytest

from oracle_lib import SCHED_2P, OracleNet, fault_threshold
from test_gpu_parity import SEED, run_parity
from test_gpu_wire import _compare, _decode_batch, _key_sorted

pytestmark = pytest.mark.gpu

ENV = "SAFE_GOSSIP_AMD_WORKLIST"


def _waves(n, R):
    rpad = max(64, 1 << (R - 1).bit_length())
    return (n * (rpad // 64) + 63) // 64


# ---------------------------------------------------------------- 1. oracle parity, forced on

@pytest.mark.parametrize("n,R", [
    (5000, 256),   # W = 4: 16 nodes per wave
    (4099, 64),    # W = 1: 64-node waves, ragged last wave
    (3001, 512),   # W = 8
    (6000, 100),   # padded to 128
])
def test_worklist_parity(engine, monkeypatch, n, R):
    # three rumors: most waves stay trivial for many rounds, and the dense
    # phase runs through the list as well
    monkeypatch.setenv(ENV, "1")
    rounds = run_parity(engine, n, R, "example")
    assert rounds > 8


# ---------------------------------------------------------------- 2. injection into a trivial wave

def test_worklist_injections(engine, monkeypatch):
    monkeypatch.setenv(ENV, "1")
    n, R = 5003, 256
    inject = {1: (0, 0), 4: (n - 1, 1), 6: (n // 2 + 3, 2)}  # before round: (node, rumor)
    net = engine.Network(n, R, seed=SEED)
    orc = OracleNet(n, R, seed=SEED)
    try:
        for rnd in range(1, 61):
            if rnd in inject:
                net.send_new(*inject[rnd])
                orc.send_new(*inject[rnd])
            rep = net.next_round()
            _, live = orc.next_round(SCHED_2P)
            assert rep.any_live == live, f"round {rnd}"
            _compare(net, orc)
            if not live:
                break
        assert not live and rnd > 8
        wl, dense, listed = net.round_path_info()
        assert (wl, dense) == (rnd - 1, 0) and 0 < listed < wl * _waves(n, R)
    finally:
        net.close()
        orc.close()


# ---------------------------------------------------------------- 3. two epochs

@pytest.mark.parametrize("mode", ["1", None])
def test_worklist_two_epochs(engine, monkeypatch, mode):
    # stale wave bytes, SibRec serials and the sticky dense switch must not
    # leak across clear()
    if mode is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, mode)
    n, R = 5000, 256
    net = engine.Network(n, R, seed=SEED)
    orc = None
    try:
        for epoch in (0, 1):
            if epoch:
                net.clear(epoch=epoch)
            orc = OracleNet(n, R, seed=SEED, epoch=epoch)
            for x, r in [(engine.origin_of(SEED, epoch, 0, n), 0), (engine.origin_of(SEED, epoch, 1, n), 1), (0, 2)]:
                net.send_new(x, r)
                orc.send_new(x, r)
            for rnd in range(1, 61):
                rep = net.next_round()
                _, live = orc.next_round(SCHED_2P)
                assert rep.any_live == live, f"epoch {epoch} round {rnd}"
                _compare(net, orc)
                if not live:
                    break
            assert not live
            wl, dense, _ = net.round_path_info()
            assert wl + dense == rnd - 1 and wl >= 1
            if mode == "1":
                assert dense == 0
            orc.close()
            orc = None
    finally:
        net.close()
        if orc is not None:
            orc.close()


# ---------------------------------------------------------------- 4, 5, 7. scale: forced on / off / auto

N_BIG, R_BIG, CHECK = 1 << 18, 256, tuple(range(1, 13)) + (22,)


def _big_run(engine, monkeypatch, mode, rounds=22, timing=False):
    if mode is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, mode)
    net = engine.Network(N_BIG, R_BIG, seed=SEED)
    try:
        if timing:
            net.set_timing(True)
        for r in range(R_BIG):
            net.send_new(engine.origin_of(SEED, 0, r, N_BIG), r)
        out = {}
        for rnd in range(1, rounds + 1):
            net.next_round(report=False)
            if rnd in CHECK:
                out[rnd] = (net.state_digest().copy(), net.statistics_all().copy())
        return out, net.round_path_info(), (net.round_traffic() if timing else None)
    finally:
        net.close()


@pytest.fixture(scope="module")
def big_off(engine):
    # the full-grid results, computed once and shared (read-only)
    mp = pytest.MonkeyPatch()
    try:
        return _big_run(engine, mp, "0")
    finally:
        mp.undo()


def _same(a, b):
    assert sorted(a) == sorted(b)
    for rnd in sorted(a):
        np.testing.assert_array_equal(a[rnd][0], b[rnd][0], err_msg=f"digest, round {rnd}")
        np.testing.assert_array_equal(a[rnd][1], b[rnd][1], err_msg=f"statistics, round {rnd}")


def test_worklist_scale_forced(engine, monkeypatch, big_off):
    # ~5000 nodes per round have in-degree > 3 here: pushers that are live
    # only in an all-A target's tail occur (InRec.kf bit 31)
    on, (wl, dense, listed), _ = _big_run(engine, monkeypatch, "1")
    off, (wl0, dense0, listed0), _ = big_off
    _same(on, off)
    assert (wl, dense) == (21, 0) and 0 < listed < 21 * _waves(N_BIG, R_BIG)
    assert (wl0, dense0, listed0) == (0, 21, 0)


def test_worklist_scale_auto(engine, monkeypatch, big_off):
    auto, (wl, dense, listed), _ = _big_run(engine, monkeypatch, None)
    _same(auto, big_off[0])
    # it began on the worklist and went over to the full grid (when is timing-dependent)
    assert wl >= 1 and dense >= 1 and wl + dense == 21 and listed > 0


def test_worklist_traffic(engine, monkeypatch):
    _, _, (b_on, l_on) = _big_run(engine, monkeypatch, "1", rounds=12, timing=True)
    _, _, (b_off, l_off) = _big_run(engine, monkeypatch, "0", rounds=12, timing=True)
    assert l_on == l_off == 11
    light = 48.125  # B per node the light pass reads (gs_kernels.h kLightNodeRead)
    assert N_BIG * light < b_on < b_off, (b_on, b_off)


# ---------------------------------------------------------------- 6. fallbacks

def test_worklist_fallback_faults(engine, monkeypatch):
    monkeypatch.setenv(ENV, "1")
    n, R, faults = 3000, 200, (0.05, 0.05, 0.05)
    net = engine.Network(n, R, seed=SEED, churn=faults[0], drop_push=faults[1], drop_pull=faults[2])
    orc = OracleNet(n, R, seed=SEED, faults=[fault_threshold(p) for p in faults])
    try:
        for r in range(0, R, 7):
            x = engine.origin_of(SEED, 0, r, n)
            net.send_new(x, r)
            orc.send_new(x, r)
        for rnd in range(1, 13):
            net.next_round()
            orc.next_round(SCHED_2P)
            np.testing.assert_array_equal(net.dump_state(), orc.dump_state())
            np.testing.assert_array_equal(net.statistics_all(), orc.statistics())
        assert net.round_path_info() == (0, 0, 0)
    finally:
        net.close()
        orc.close()


def test_worklist_fallback_external_rpc(engine, monkeypatch):
    monkeypatch.setenv(ENV, "1")
    n, R = 2000, 64
    net = engine.Network(n, R, seed=SEED)
    orc = OracleNet(n, R, seed=SEED)
    try:
        net.send_new(7, 0)
        orc.send_new(7, 0)
        for rnd in range(1, 8):
            if rnd == 3:  # an external peer pushes rumor 1 to an all-A node of round 2
                y, peer = n - 5, n + 1
                got = net.handle_received(y, peer, engine.rpc_encode(False, net.rumor_key(1), 1))
                exp = orc.receive(y, peer, True, 1, 1)
                assert _decode_batch(engine, net, got, pull=True) == _key_sorted(net, exp)
            net.next_round()
            orc.next_round(SCHED_2P)
            _compare(net, orc)
        wl, dense, _ = net.round_path_info()
        assert (wl, dense) == (5, 1)  # rounds 2..7 deliver; round 3 carried the RPC
    finally:
        net.close()
        orc.close()


def test_worklist_fallback_slice(engine, monkeypatch):
    monkeypatch.setenv(ENV, "1")
    from safe_gossip_amd.sliced import SlicedNetwork
    n, R = 700, 256  # two slices of 128 rumors: the gather path, W = 2
    net = SlicedNetwork(n, R, 2, seed=SEED, transport="local")
    orc = OracleNet(n, R, seed=SEED)
    try:
        for x, r in [(engine.origin_of(SEED, 0, 0, n), 0), (engine.origin_of(SEED, 0, 200, n), 200), (0, 2)]:
            net.send_new(x, r)
            orc.send_new(x, r)
        for rnd in range(1, 9):
            net.next_round()
            orc.next_round(SCHED_2P)
            np.testing.assert_array_equal(net.dump_state(), orc.dump_state())
            np.testing.assert_array_equal(net.statistics_all(), orc.statistics())
        for s in net.slices:
            assert s.net.round_path_info() == (0, 0, 0)
    finally:
        net.close()
        orc.close()
