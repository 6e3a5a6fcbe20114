"""Scenarios that drive the 5-bit state field `b` (B.round / C.rounds_in_state_b,
planes 3..7 of the packed state) up to 31, and the median rule across its exact
ties -- shared by tests/test_state_edges_oracle.py (CPU: the oracle against a
plain restatement of MessageState::next_round, plus what each scenario covers)
and tests/test_gpu_state_edges.py (GPU: every engine layout against the oracle).

TEST INFRASTRUCTURE ONLY.

Two ways to get there without any product change:

* staggered: drop most internal batches (drop_push 0.95, drop_pull 0.8), so
  cells hear little and stay B for up to max_rounds rounds, with injections
  spread over rounds 1..6 so that the columns of one node differ;
* external RPCs with every internal batch dropped (drop 1.0 / 1.0): the
  records and |peers_in_this_round| of a node are exactly what the test's
  peers outside the network hand it, so every cell follows a script.

What a run covered is read from consecutive oracle dumps alone (Coverage), so
it is a property of the inputs, not of the engine layout that replays them.
"""
import numpy as np

from oracle_lib import SCHED_2P, SCHED_SEQ, OracleNet, fault_threshold
from test_gpu_parity import SEED

TAG_A, TAG_B, TAG_C, TAG_D = 0, 1, 2, 3
CODE_NEW_B = (TAG_B << 14) | (1 << 7)   # MessageState::new / new_from_peer below counter_max
CODE_NEW_C = TAG_C << 14                # new_from_peer at or above counter_max
CODE_D = TAG_D << 14


def next_code(code, rec, psize, params):
    """MessageState::next_round (src/message_state.rs:86-171) on the dumps.

    code  = tag<<14 | f2<<7 | f1 (B: f1 round, f2 our_counter; C: f1
            rounds_in_state_b, f2 round), as dump_state gives it;
    rec   = anyC<<15 | cnt2<<7 | cnt1, the summary of B.peer_counters;
    psize = |peers_in_this_round|: every recorded peer is one of them, so after
            the 0-fill peer_counters has psize entries, and those not counted
            as ">= own" are "less".
    Returns the next code."""
    cmax, maxc, maxr = params
    tag, f1, f2 = code >> 14, code & 0x7F, (code >> 7) & 0x7F
    if tag == TAG_B:
        rnd, our = f1 + 1, f2
        if rnd >= maxr:
            return CODE_D
        if rec >> 15:                      # a peer in state C
            return (TAG_C << 14) | rnd
        ge = (rec & 0x7F) if our == 1 else ((rec >> 7) & 0x7F)
        less = psize - ge
        if ge > less:
            our += 1
        if our >= cmax:
            return (TAG_C << 14) | rnd
        return (TAG_B << 14) | (our << 7) | rnd
    if tag == TAG_C:
        rib, rnd = f1, f2 + 1
        if rnd + rib >= maxr:
            return CODE_D
        if rnd >= maxc:
            return CODE_D
        return (TAG_C << 14) | (rnd << 7) | rib
    return code                            # D stays D; A has no MessageState


class Coverage:
    """What the transitions between consecutive oracle dumps exercised."""

    def __init__(self, votes=False):
        self.b_rounds = {1: set(), 2: set()}   # B rounds seen, per our_counter
        self.ribs = set()                      # rounds_in_state_b seen in C
        self.b_to_d = {1: 0, 2: 0}             # B -> D by the round limit, per our_counter
        self.c_to_d_rib = set()                # ribs at which C -> D by round + rib
        self.c_to_d_maxc = 0                   # C -> D by max_c_rounds
        self.c_by_anyc = set()                 # ribs entered because a peer was in C
        self.c_by_counter = set()              # ribs entered because our_counter reached counter_max
        self.votes = set() if votes else None  # (our_counter, |P|, ge) of B cells that voted
        self.cells = 0                         # transitions checked

    def see(self, state):
        """B rounds and ribs present in one dump."""
        for c in np.unique(state):
            c = int(c)
            if c >> 14 == TAG_B:
                self.b_rounds.setdefault((c >> 7) & 0x7F, set()).add(c & 0x7F)
            elif c >> 14 == TAG_C:
                self.ribs.add(c & 0x7F)

    def _transition(self, code, rec, psize, post, params):
        cmax, maxc, maxr = params
        tag, f1, f2 = code >> 14, code & 0x7F, (code >> 7) & 0x7F
        if tag == TAG_B:
            if post == CODE_D:
                self.b_to_d[f2] = self.b_to_d.get(f2, 0) + 1
                return
            if self.votes is not None:
                self.votes.add((f2, psize, (rec & 0x7F) if f2 == 1 else ((rec >> 7) & 0x7F)))
            if post >> 14 == TAG_C:
                (self.c_by_anyc if rec >> 15 else self.c_by_counter).add(post & 0x7F)
        elif tag == TAG_C and post == CODE_D:
            if f2 + 1 + f1 >= maxr:
                self.c_to_d_rib.add(f1)
            else:
                self.c_to_d_maxc += 1


def dumps(orc):
    rec, ps = orc.dump_records()
    return orc.dump_state(), rec, ps


def check_step(cov, pre, post_state, params, offline=None, injected=()):
    """One Gossip::next_round per node between two oracle dumps: `pre` =
    (state, records, |P|) before it (after the last RPC of the round before),
    `post_state` after the round's deliveries.  Every cell of an online node
    must be next_code's; deliveries change no existing state, they only create
    (new_from_peer).  send_new replaces the cell by a fresh B before the
    transition; a node that churn takes offline keeps its cells."""
    state, rec, ps = (a.copy() for a in pre)
    for x, r in injected:
        state[x, r] = CODE_NEW_B
        rec[x, r] = 0
    n, R = state.shape
    if offline is not None and offline.any():
        np.testing.assert_array_equal(post_state[offline], state[offline])
        on = ~offline
        state, rec, ps, post_state = state[on], rec[on], ps[on], post_state[on]
    assert int(ps.max(initial=0)) < (1 << 15)
    key = (state.astype(np.uint64) | (rec.astype(np.uint64) << np.uint64(16))
           | (np.broadcast_to(ps[:, None], state.shape).astype(np.uint64) << np.uint64(32))
           | (post_state.astype(np.uint64) << np.uint64(48)))
    for k in np.unique(key):
        k = int(k)
        code, rc, p, post = k & 0xFFFF, (k >> 16) & 0xFFFF, (k >> 32) & 0xFFFF, k >> 48
        if code >> 14 == TAG_A:
            assert post in (0, CODE_NEW_B, CODE_NEW_C), f"created as {post:#06x}"
            continue
        exp = next_code(code, rc, p, params)
        if post != exp:
            at = tuple(np.argwhere(key == np.uint64(k))[0])
            raise AssertionError(f"online cell {at}: {code:#06x} rec {rc:#06x} |P| {p} -> oracle {post:#06x}, "
                                 f"restated {exp:#06x}")
        cov._transition(code, rc, p, post, params)
    cov.cells += int(state.size)
    cov.see(post_state)


# ---------------------------------------------------------------- staggered, faults on

F_HEAVY = (0.0, 0.95, 0.8)

# name -> (n, R, params, (churn, drop_push, drop_pull)); the engine layouts
# that replay each one are listed in tests/test_gpu_state_edges.py
STAGGERED = {
    "500x16": (500, 16, (3, 3, 32), F_HEAVY),
    "999x7-churn": (999, 7, (3, 3, 31), (0.05, 0.93, 0.7)),
    "1030x1": (1030, 1, (3, 3, 32), F_HEAVY),
    "101x32": (101, 32, (3, 3, 32), F_HEAVY),
    "300x64": (300, 64, (3, 3, 32), F_HEAVY),
    "130x256": (130, 256, (3, 3, 32), F_HEAVY),
    "500x16-max17": (500, 16, (3, 3, 17), F_HEAVY),
    "500x16-max16": (500, 16, (3, 3, 16), F_HEAVY),
    "500x16-cmax2": (500, 16, (2, 2, 32), F_HEAVY),
    "5000x16": (5000, 16, (3, 3, 32), F_HEAVY),
}
SEQ_TOO = ("500x16", "300x64")  # also replayed under the SEQ schedule


def staggered_plan(n, R):
    """{round: [(node, rumor)]}: send_new before round 1 + ((7x + 3r) mod 6),
    for every cell with (x + r) mod 4 != 0 (those learn the rumor from peers)."""
    plan = {}
    for x in range(n):
        for r in range(R):
            if (x + r) % 4:
                plan.setdefault(1 + (7 * x + 3 * r) % 6, []).append((x, r))
    return plan


def run_staggered(n, R, params, faults, schedule="2P", net=None, compare=None, cov=None, cap=90):
    """The oracle (and `net`, compared after every round) until the oracle
    reports nothing live, round 7 at the earliest, `cap` at the latest."""
    osched = SCHED_SEQ if schedule == "SEQ" else SCHED_2P
    orc = OracleNet(n, R, seed=SEED, params=params, faults=[fault_threshold(p) for p in faults])
    plan = staggered_plan(n, R)
    pre = (np.zeros((n, R), np.uint16), np.zeros((n, R), np.uint16), np.zeros(n, np.uint32))
    try:
        if net is not None:
            assert net.params == orc.params == tuple(params)
        for rnd in range(1, cap + 1):
            inj = plan.get(rnd, ())
            for x, r in inj:
                orc.send_new(x, r)
                if net is not None:
                    net.send_new(x, r)
            rc, live = orc.next_round(osched)
            assert rc == 0
            off = orc.offline(rnd) if faults[0] > 0 else None
            if net is not None:
                rep = net.next_round()
                assert rep.round == rnd and rep.any_live == live, f"round {rnd}: any_live"
                try:
                    compare(net, orc, off)
                except AssertionError as e:
                    raise AssertionError(f"round {rnd}: {e}") from None
            if cov is not None:
                post = dumps(orc)
                check_step(cov, pre, post[0], params, off, inj)
                pre = post
            if rnd >= 7 and not live:
                break
        return rnd
    finally:
        orc.close()


def staggered_conditions(cov, params):
    cmax, maxc, maxr = params
    ocs = (1, 2) if cmax >= 3 else (1,)      # counter_max 2: our_counter 2 is never a B state
    assert set(range(1, maxr)) <= cov.b_rounds[1], sorted(set(range(1, maxr)) - cov.b_rounds[1])
    if 2 in ocs:
        assert set(range(2, maxr)) <= cov.b_rounds[2], sorted(set(range(2, maxr)) - cov.b_rounds[2])
    assert set(range(10, maxr)) <= cov.ribs, sorted(set(range(10, maxr)) - cov.ribs)
    for oc in ocs:
        assert cov.b_to_d[oc] > 0, f"no B->D at our_counter {oc}"
    # C.round stays below max_c_rounds, so round + 1 + rib reaches max_rounds only
    # for rib >= max_rounds - max_c_rounds: the last three ribs when that is 3
    assert set(range(maxr - maxc, maxr)) <= cov.c_to_d_rib, sorted(cov.c_to_d_rib)


# ---------------------------------------------------------------- external RPCs, every internal batch dropped

F_ALL = (0.0, 1.0, 1.0)


def run_ext(n, R, params, inject, rpcs_after, rounds, schedule="2P", net=None, compare=None,
            hand_off=None, cov=None):
    """send_new(`inject`), then `rounds` rounds; after round t the RPCs
    rpcs_after(t) = [(node, peer, push, rumor or -1, counter)] go through
    Gossip::receive of the oracle and, by hand_off(net, rpcs, expected
    responses), of the engine, which is compared after the round and after the
    hand-off."""
    osched = SCHED_SEQ if schedule == "SEQ" else SCHED_2P
    orc = OracleNet(n, R, seed=SEED, params=params, faults=[fault_threshold(p) for p in F_ALL])
    pre = (np.zeros((n, R), np.uint16), np.zeros((n, R), np.uint16), np.zeros(n, np.uint32))
    try:
        for x, r in inject:
            orc.send_new(x, r)
            if net is not None:
                net.send_new(x, r)
        for rnd in range(1, rounds + 1):
            rc, _ = orc.next_round(osched)
            assert rc == 0
            if net is not None:
                net.next_round()
                try:
                    compare(net, orc)
                except AssertionError as e:
                    raise AssertionError(f"round {rnd}: {e}") from None
            if cov is not None:
                check_step(cov, pre, orc.dump_state(), params, None, inject if rnd == 1 else ())
            rpcs = rpcs_after(rnd)
            if rpcs:
                exp = [orc.receive(*rpc) for rpc in rpcs]
                if net is not None:
                    try:
                        hand_off(net, rpcs, exp)
                        compare(net, orc)
                    except AssertionError as e:
                        raise AssertionError(f"hand-off after round {rnd}: {e}") from None
            if cov is not None:
                pre = dumps(orc)
                if rpcs:  # every internal batch is dropped: |P| is the external peers alone
                    heard = np.zeros(n, np.uint32)
                    for y, ps in _peer_sets(rpcs).items():
                        heard[y] = len(ps)
                    np.testing.assert_array_equal(pre[2], heard)
    finally:
        orc.close()


def _peer_sets(rpcs):
    out = {}
    for y, peer, *_ in rpcs:
        out.setdefault(y, set()).add(peer)
    return out


# vote grid: node y hears from E_y = y + 1 peers; on column c, min(g(c), E_y)
# of them send a copy that votes ">= own", the others are 0-filled ("less")

VOTE_N, VOTE_PARAMS, VOTE_ROUNDS = 40, (3, 3, 14), 16
VOTE_COUNTERS = (1, 2, 2)   # the copies' counter, per stage (hand-off after round 1, 2, 3)


def vote_g(R, stage, E, c):
    if R >= 64:   # every ge 0..E at every E, the stages rotated against each other
        return min((c + 21 * (stage - 1)) % R, E)
    # narrower: the columns centred on the tie 2 ge = E.  A cell reaches
    # our_counter 2 by a majority (offset >= +1 from the centre), so the later
    # stages shift the columns by 2 to bring the same cells back to -1, 0, +1
    return min(max(E // 2 - R // 2 + (c - 2 * (stage - 1)) % R, 0), E)


def vote_rpcs(n, R, stage):
    ctr = VOTE_COUNTERS[stage - 1]
    order = np.random.default_rng(1000 * R + stage).permutation(n)
    out = []
    for i in order:          # peer by peer, the nodes interleaved
        i = int(i)
        for y in range(i, n):    # E_y = y + 1 > i
            cols = [c for c in range(R) if i < vote_g(R, stage, y + 1, c)]
            if not cols:         # a peer of this round with no copy
                out.append((y, n + 1 + i, True, -1, 0))
            out += [(y, n + 1 + i, True, c, ctr) for c in cols]
    return out


def run_votes(R, **kw):
    n = VOTE_N
    run_ext(n, R, VOTE_PARAMS, [(x, r) for x in range(n) for r in range(R)],
            lambda rnd: vote_rpcs(n, R, rnd) if rnd <= len(VOTE_COUNTERS) else [], VOTE_ROUNDS, **kw)


def vote_conditions(cov, R):
    n = VOTE_N
    for oc in (1, 2):
        if R >= 64:   # the full grid
            want = {(oc, p, ge) for p in range(1, n + 1) for ge in range(p + 1)}
            assert len(want) == 860
        else:         # the ties and one vote to either side
            want = {(oc, p, ge) for p in range(1, n + 1) for ge in range(p + 1) if abs(2 * ge - p) <= 2}
        assert want <= cov.votes, f"our_counter {oc}: {len(want - cov.votes)} of {len(want)} missing, " \
                                  f"e.g. {sorted(want - cov.votes)[:5]}"


# scripted lifetimes: one external peer per node and round (|P| = 1: its copy
# is a majority, every other B cell of the node sees one "less" vote and stays)

LIFE_N, LIFE_PARAMS, LIFE_ROUNDS = 70, (3, 3, 32), 36


def lifetime_plan(n, R):
    """64 scripts ("virtual columns"), folded onto R columns by node group
    when R < 64, rotated by y mod 3 so that neighbouring nodes differ.
      v in 0..30:  B -> C because a peer is in C (one counter-255 copy), at
                   rounds_in_state_b = 1 + (v + 10 (y mod 3)) mod 31, i.e. 1..31;
      v in 32..62: B -> C by the counter, two one-peer majorities in a row
                   ending at rib = 2 + (v - 32 + 10 (y mod 3)) mod 31, i.e.
                   2..32 -- "32" is past the limit: that cell goes B -> D at
                   our_counter 2;
      v = 31, 63:  never touched: B -> D at our_counter 1.
    A cell is B{round t} after round t when it was injected before round 1, so
    rib 1 (anyC) and rib 2 (counter) need a cell younger than the network: it
    is created after round 1 by the peer's first copy (new_from_peer, which is
    not recorded) and the same peer's second copy is the recorded one.
    Returns (injections, {round: rpcs after it})."""
    assert 64 % R == 0
    inject, after = [], {}
    for y in range(n):
        s, fold = y % 3, (y // 3) % (64 // R)
        mine = {}
        for j in range(R):
            v = j + R * fold
            if v in (31, 63):
                inject.append((y, j))
            elif v < 31:
                rib = 1 + (v + 10 * s) % 31
                if rib == 1:
                    mine.setdefault(1, []).extend([(j, 1), (j, 255)])
                else:
                    inject.append((y, j))
                    mine.setdefault(rib - 1, []).append((j, 255))
            else:
                rib = 2 + (v - 32 + 10 * s) % 31
                if rib == 2:   # B{0} after round 1, B{1, our_counter 2} after round 2
                    mine.setdefault(1, []).extend([(j, 1), (j, 1)])
                    mine.setdefault(2, []).append((j, 2))
                else:
                    inject.append((y, j))
                    mine.setdefault(rib - 2, []).append((j, 1))
                    mine.setdefault(rib - 1, []).append((j, 2))
        for rnd, copies in mine.items():
            peer = n + 1 + (y + rnd) % 7
            push = (y + rnd) % 4 != 3   # some peers hand their copies over as Pull RPCs
            after.setdefault(rnd, []).extend((y, peer, push, j, ctr) for j, ctr in copies)
    return inject, after


def run_lifetimes(R, **kw):
    inject, after = lifetime_plan(LIFE_N, R)
    run_ext(LIFE_N, R, LIFE_PARAMS, inject, lambda rnd: after.get(rnd, []), LIFE_ROUNDS, **kw)


def lifetime_conditions(cov):
    assert set(range(1, 32)) <= cov.c_by_anyc, sorted(set(range(1, 32)) - cov.c_by_anyc)
    assert set(range(2, 32)) <= cov.c_by_counter, sorted(set(range(2, 32)) - cov.c_by_counter)
    assert {29, 30, 31} <= cov.c_to_d_rib and cov.c_to_d_maxc > 0
    assert cov.b_to_d[1] > 0 and cov.b_to_d[2] > 0
    assert set(range(1, 32)) <= cov.b_rounds[1] and set(range(1, 32)) <= cov.ribs
