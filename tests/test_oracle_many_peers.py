"""The CPU oracle at vote counts far above what the simulated network itself
produces: one hub node hears from 100 peers outside the network in one round
(Gossip::receive through or_receive), and MessageState::next_round's median
rule (src/message_state.rs:94-147) is restated here in plain Python and
compared with the oracle's next state for every number of ">= own" votes
0..100, at our_counter 1 and 2, with and without one counter-255 copy.  Also
pins or_dump_records' 7-bit counts (cnt1 / cnt2) up to 100.

The GPU tests of tests/test_gpu_ext_votes.py use the oracle as their
reference at these counts; this file is what makes it one.
"""
import pytest

from oracle_lib import SCHED_2P, OracleNet

E = 100                # external peers
N, HUB = 64, 5
R = E + 1              # column j: m_j = j peers vote ">= own"


def restated_next_round(our_counter, rnd, counters, n_peers, cmax, maxr):
    """MessageState::next_round on B{round, our_counter, peer_counters}:
    `counters` = the recorded values, n_peers = |peers_in_this_round| (every
    recorded peer is one of them).  Returns (tag, round, our_counter) for B,
    (tag, round, rounds_in_state_b) for C, ("D",)."""
    rnd += 1
    if rnd >= maxr:
        return ("D",)
    values = list(counters) + [0] * (n_peers - len(counters))  # the 0-fill
    less = ge = 0
    for v in values:
        if v < our_counter:
            less += 1
        elif v >= cmax:
            return ("C", 0, rnd)
        else:
            ge += 1
    if ge > less:
        our_counter += 1
    if our_counter >= cmax:
        return ("C", 0, rnd)
    return ("B", rnd, our_counter)


def _decode(code):
    tag = "ABCD"[code >> 14]
    if tag in "AD":
        return (tag,)
    return (tag, (code & 0x7F) if tag == "B" else (code >> 7) & 0x7F, (code >> 7) & 0x7F if tag == "B" else code & 0x7F)


def _internal(rec):
    """The recorded values behind one or_dump_records entry."""
    c1, c2, any_c = rec & 0x7F, (rec >> 7) & 0x7F, rec >> 15
    return [2] * c2 + [1] * (c1 - c2) + [255] * any_c


def _hand_off(orc, ge_ctr, less_ctr, with_c):
    """Column j: peers 0..j-1 push (r_j, ge_ctr); of the others every second
    one pushes less_ctr (recorded, unless None), the rest push nothing for
    r_j and are 0-filled.  Column R-1 makes every peer a peer of this round.
    Returns the values recorded per column."""
    recorded = [[] for _ in range(R)]
    for i in range(E):
        for j in range(R):
            if i < j:
                ctr = ge_ctr
            elif less_ctr is not None and (i - j) % 2 == 0:
                ctr = less_ctr
            else:
                continue
            orc.receive(HUB, N + 1 + i, True, j, ctr)
            recorded[j].append(ctr)
    if with_c:
        for j in range(R):
            orc.receive(HUB, N + 1 + E, j % 2 == 0, j, 255)  # Push and Pull copies alike
            recorded[j].append(255)
    return recorded


@pytest.mark.parametrize("with_c", [False, True], ids=["noC", "C"])
@pytest.mark.parametrize("our_counter,params", [(1, (3, 3, 14)), (2, (3, 3, 14)), (2, (3, 3, 3))],
                         ids=["oc1", "oc2", "oc2-maxrounds"])
def test_median_rule_up_to_100_votes(oracle, our_counter, params, with_c):
    cmax, _, maxr = params
    orc = OracleNet(N, R, params=params)
    try:
        for r in range(R):
            orc.send_new(HUB, r)
        orc.next_round(SCHED_2P)
        if our_counter == 2:  # every peer votes ">= own": all columns bump to 2
            for i in range(E):
                for j in range(R):
                    orc.receive(HUB, N + 1 + i, True, j, 1)
            orc.next_round(SCHED_2P)
        before = orc.dump_state()[HUB]
        rec0, ps0 = orc.dump_records()
        rnd0 = our_counter  # next_round calls so far (the injecting one included)
        for j in range(R):
            assert _decode(int(before[j])) == ("B", rnd0, our_counter)
        # ">=" copies carry our_counter; "less" copies our_counter - 1 (0 is
        # recorded too, src/message_state.rs:77-83, and counts in no cnt)
        recorded = _hand_off(orc, our_counter, our_counter - 1, with_c)
        n_peers = int(ps0[HUB]) + E + (1 if with_c else 0)
        rec, ps = orc.dump_records()
        assert int(ps[HUB]) == n_peers
        top = 0
        for j in range(R):
            vals = _internal(int(rec0[HUB, j])) + recorded[j]
            cnt1 = sum(1 for v in vals if 1 <= v < cmax)
            cnt2 = sum(1 for v in vals if v == 2 and 2 < cmax)
            any_c = int(any(v >= cmax for v in vals))
            assert int(rec[HUB, j]) == (any_c << 15) | (cnt2 << 7) | cnt1, f"column {j}"
            top = max(top, cnt1, cnt2)
        assert top >= E  # the 7-bit counts were driven to 100
        orc.next_round(SCHED_2P)
        after = orc.dump_state()[HUB]
        seen = set()
        for j in range(R):
            vals = _internal(int(rec0[HUB, j])) + recorded[j]
            exp = restated_next_round(our_counter, rnd0, vals, n_peers, cmax, maxr)
            assert _decode(int(after[j])) == exp, f"column {j}: {len(recorded[j])} recorded"
            seen.add(exp)
        # not vacuous: both outcomes of the median rule occur
        if rnd0 + 1 >= maxr:
            assert seen == {("D",)}
        elif with_c:
            assert seen == {("C", 0, rnd0 + 1)}
        elif our_counter == 1:
            assert seen == {("B", 2, 1), ("B", 2, 2)}
        else:
            assert seen == {("B", 3, 2), ("C", 0, 3)}
    finally:
        orc.close()


def test_restatement_edges():
    # ge > less is strict; 0-filled peers vote "less"; a C copy wins whatever the votes
    assert restated_next_round(1, 0, [1] * 50, 100, 3, 14) == ("B", 1, 1)
    assert restated_next_round(1, 0, [1] * 51, 100, 3, 14) == ("B", 1, 2)
    assert restated_next_round(1, 0, [0] * 99 + [255], 100, 3, 14) == ("C", 0, 1)
    assert restated_next_round(2, 5, [2] * 32, 62, 3, 14) == ("C", 0, 6)
    assert restated_next_round(2, 5, [2] * 31 + [1] * 31, 62, 3, 14) == ("B", 6, 2)
    assert restated_next_round(1, 12, [1] * 64, 64, 3, 14) == ("B", 13, 2)
    assert restated_next_round(1, 13, [255], 1, 3, 14) == ("D",)
